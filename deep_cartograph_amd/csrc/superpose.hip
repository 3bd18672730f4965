// Optimal rigid superposition of every frame of a trajectory (analyze_geometry: RMSD, average structure, RMSF; the
// primitive of coordinate features and trajectory alignment): fit on one atom set, transform and measure on another.
//
// One fused launch.  The grid is capped at DCV_SUPERPOSE_MAX_GROUPS workgroups that stride over tiles of frames.  A
// workgroup stages the union of the fit and the selected atoms of its tile into LDS once (stage.h, the staging of
// featurize.hip) and does everything else from there, in float64:
//   phase A  a group of `fl` lanes (16 at the full tile of 16 frames) owns a frame: weighted centroid of the fit atoms,
//            the 3 x 3 correlation of the CENTRED coordinates with the centred reference -- the 3 + 9 sums reduced over
//            the lanes of the group with xor shuffles, after which every lane holds the same bits --, the rotation
//            (horn.h: Jacobi on Horn's 4 x 4 matrix, solved redundantly by the lanes of the group), then the two RMSDs
//            from the residuals of the transformed coordinates (never from G_a + G_b - 2 lambda, which loses half the
//            digits near 0).  Lane 0 of the group writes the transform and RMSD rows and parks the transform in LDS;
//   phase B  (aligned coordinates or moments wanted) a thread owns a selected atom and walks the frames of the tile:
//            aligned = (x - c_mob) . R + c_ref goes out rounded once to float32, d = aligned - sel_ref is summed (d and
//            d^2) in registers over the tile and then added to the thread's own float64 entries of the workgroup's
//            moment partials in LDS.
// At the end each workgroup writes its partials once; a second small launch adds them in workgroup order.  Tiles are
// dealt to workgroups statically, so the moments are bit-identical from run to run.  No atomics.
#include <cmath>
#include <vector>

#include "common.h"
#include "horn.h"
#include "stage.h"

namespace dcv {

constexpr int kSupXf = 16;   // doubles of a transform row: R (9, row-major), c_mob (3), c_ref (3), fit RMSD

struct SupArgs {
    StageArgs st;
    const int32_t* fit_slot;   // n_fit LDS slots
    const double* fit_rec;     // n_fit x 4: centred reference x, y, z and the weight
    const int32_t* sel_slot;   // n_sel LDS slots
    const double* sel_ref;     // n_sel x 3 or NULL
    int32_t n_fit, n_sel;
    double inv_w;              // 1 / sum of the weights
    double c_ref[3];
    int32_t fl;                // lanes per frame in phase A (power of two, <= 64)
    int64_t n_tiles;
    int32_t xf_off, mom_off;   // byte offsets of the parked transforms and of the moment partials in LDS
    double* transform;         // n x 16 or NULL
    double* rmsd;              // n x 2 or NULL
    float* aligned;            // n x lda or NULL
    int64_t lda;
    double* partials;          // gridDim.x x n_sel x 6 or NULL: per selected atom sum d (3), sum d^2 (3)
};

template <int N>
__device__ __forceinline__ void group_sum(double (&v)[N], int fl) {
    for (int m = fl >> 1; m > 0; m >>= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] += __shfl_xor(v[i], m, kWave);
    }
}

__global__ __launch_bounds__(kStageThreads) void superpose_kernel(const SupArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lds = reinterpret_cast<float*>(smem);
    double* xf = reinterpret_cast<double*>(smem + a.xf_off);
    double* mom = reinterpret_cast<double*>(smem + a.mom_off);
    const int t = threadIdx.x;
    const int fl = a.fl, gl = t & (fl - 1), grp = t / fl, groups = kStageThreads / fl;
    const int las = a.st.las, lcs = a.st.lcs;
    const bool phase_b = a.aligned != nullptr || a.partials != nullptr;
    if (a.partials)
        for (int e = t; e < a.n_sel * 6; e += kStageThreads) mom[e] = 0.0;   // phase B, behind the barrier after staging: atom i belongs to thread i % 256

    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t f0 = tile * a.st.tile;
        const int nf = a.st.n_frames - f0 < a.st.tile ? (int)(a.st.n_frames - f0) : a.st.tile;
        stage_tile(a.st, f0, nf, lds);
        __syncthreads();

        // ---- phase A: a group of fl lanes per frame (whole groups take the branch, so the shuffles stay inside active lanes)
        for (int f = grp; f < nf; f += groups) {
            const float* lf = lds + f * a.st.lfs;
            double c[3] = {0.0, 0.0, 0.0};
            for (int i = gl; i < a.n_fit; i += fl) {
                const int s = a.fit_slot[i] * las;
                const double w = a.fit_rec[4 * (int64_t)i + 3];
                c[0] += w * (double)lf[s]; c[1] += w * (double)lf[s + lcs]; c[2] += w * (double)lf[s + 2 * lcs];
            }
            group_sum(c, fl);
            c[0] *= a.inv_w; c[1] *= a.inv_w; c[2] *= a.inv_w;
            double S[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int i = gl; i < a.n_fit; i += fl) {
                const int s = a.fit_slot[i] * las;
                const double* r = a.fit_rec + 4 * (int64_t)i;
                const double w = r[3];
                const double x0 = w * ((double)lf[s] - c[0]), x1 = w * ((double)lf[s + lcs] - c[1]), x2 = w * ((double)lf[s + 2 * lcs] - c[2]);
                S[0] += x0 * r[0]; S[1] += x0 * r[1]; S[2] += x0 * r[2];
                S[3] += x1 * r[0]; S[4] += x1 * r[1]; S[5] += x1 * r[2];
                S[6] += x2 * r[0]; S[7] += x2 * r[1]; S[8] += x2 * r[2];
            }
            group_sum(S, fl);
            double R[9];
            horn_rotation(S, R);
            // fit RMSD and RMSD of the selection from the residuals of the transformed coordinates
            double e[2] = {0.0, 0.0};
            for (int i = gl; i < a.n_fit; i += fl) {
                const int s = a.fit_slot[i] * las;
                const double* r = a.fit_rec + 4 * (int64_t)i;
                const double x0 = (double)lf[s] - c[0], x1 = (double)lf[s + lcs] - c[1], x2 = (double)lf[s + 2 * lcs] - c[2];
                const double d0 = x0 * R[0] + x1 * R[3] + x2 * R[6] - r[0];
                const double d1 = x0 * R[1] + x1 * R[4] + x2 * R[7] - r[1];
                const double d2 = x0 * R[2] + x1 * R[5] + x2 * R[8] - r[2];
                e[0] += r[3] * (d0 * d0 + d1 * d1 + d2 * d2);
            }
            if (a.sel_ref && a.rmsd) {
                for (int i = gl; i < a.n_sel; i += fl) {
                    const int s = a.sel_slot[i] * las;
                    const double* r = a.sel_ref + 3 * (int64_t)i;
                    const double x0 = (double)lf[s] - c[0], x1 = (double)lf[s + lcs] - c[1], x2 = (double)lf[s + 2 * lcs] - c[2];
                    const double d0 = x0 * R[0] + x1 * R[3] + x2 * R[6] + a.c_ref[0] - r[0];
                    const double d1 = x0 * R[1] + x1 * R[4] + x2 * R[7] + a.c_ref[1] - r[1];
                    const double d2 = x0 * R[2] + x1 * R[5] + x2 * R[8] + a.c_ref[2] - r[2];
                    e[1] += d0 * d0 + d1 * d1 + d2 * d2;
                }
            }
            group_sum(e, fl);
            if (gl == 0) {
                const double fit_rmsd = sqrt(e[0] * a.inv_w);
                if (a.rmsd) {
                    a.rmsd[2 * (f0 + f)] = fit_rmsd;
                    a.rmsd[2 * (f0 + f) + 1] = a.sel_ref ? sqrt(e[1] / (double)a.n_sel) : 0.0;
                }
                if (a.transform) {
                    double* o = a.transform + kSupXf * (f0 + f);
#pragma unroll
                    for (int k = 0; k < 9; ++k) o[k] = R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) { o[9 + k] = c[k]; o[12 + k] = a.c_ref[k]; }
                    o[15] = fit_rmsd;
                }
                if (phase_b) {
                    double* o = xf + 12 * f;
#pragma unroll
                    for (int k = 0; k < 9; ++k) o[k] = R[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) o[9 + k] = c[k];
                }
            }
        }

        // ---- phase B: a thread per selected atom, over the frames of the tile
        if (phase_b) {
            __syncthreads();
            for (int i = t; i < a.n_sel; i += kStageThreads) {
                const int s = a.sel_slot[i] * las;
                double y0 = 0.0, y1 = 0.0, y2 = 0.0;
                if (a.partials) { y0 = a.sel_ref[3 * (int64_t)i]; y1 = a.sel_ref[3 * (int64_t)i + 1]; y2 = a.sel_ref[3 * (int64_t)i + 2]; }
                double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int f = 0; f < nf; ++f) {
                    const float* lf = lds + f * a.st.lfs;
                    const double* o = xf + 12 * f;
                    const double x0 = (double)lf[s] - o[9], x1 = (double)lf[s + lcs] - o[10], x2 = (double)lf[s + 2 * lcs] - o[11];
                    const double p0 = x0 * o[0] + x1 * o[3] + x2 * o[6] + a.c_ref[0];
                    const double p1 = x0 * o[1] + x1 * o[4] + x2 * o[7] + a.c_ref[1];
                    const double p2 = x0 * o[2] + x1 * o[5] + x2 * o[8] + a.c_ref[2];
                    if (a.aligned) {
                        float* q = a.aligned + (f0 + f) * a.lda + 3 * (int64_t)i;
                        q[0] = (float)p0; q[1] = (float)p1; q[2] = (float)p2;
                    }
                    const double d0 = p0 - y0, d1 = p1 - y1, d2 = p2 - y2;
                    m[0] += d0; m[1] += d1; m[2] += d2;
                    m[3] += d0 * d0; m[4] += d1 * d1; m[5] += d2 * d2;
                }
                if (a.partials) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) mom[6 * i + k] += m[k];
                }
            }
        }
        __syncthreads();   // the next tile overwrites the coordinates and the parked transforms
    }
    if (a.partials) {
        double* o = a.partials + (int64_t)blockIdx.x * a.n_sel * 6;
        for (int e = t; e < a.n_sel * 6; e += kStageThreads) o[e] = mom[e];   // behind the barrier that closes the last tile
    }
}

// moments[e] = sum over the workgroups' partials, in workgroup order
__global__ __launch_bounds__(256) void superpose_moments_kernel(const double* partials, int groups, int n, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += partials[(int64_t)g * n + e];
    // entry e = 6 i + k of atom i: k < 3 the sum of d_k, k >= 3 the sum of d_k^2; out is n_sel x 3 x 2
    const int i = e / 6, k = e - 6 * i;
    out[6 * i + 2 * (k % 3) + k / 3] = s;
}

struct SupLayout {
    size_t fit_slot, fit_rec, sel_slot, sel_ref, used, partials, total;
};

static SupLayout sup_layout(int64_t n_frames, int32_t n_atoms, int32_t n_fit, int32_t n_sel) {
    SupLayout l{};
    size_t o = 0;
    l.fit_slot = o; o += align_up((size_t)n_fit * sizeof(int32_t), 256);
    l.fit_rec = o; o += align_up((size_t)n_fit * 4 * sizeof(double), 256);
    l.sel_slot = o; o += align_up((size_t)n_sel * sizeof(int32_t), 256);
    l.sel_ref = o; o += align_up((size_t)n_sel * 3 * sizeof(double), 256);
    l.used = o; o += align_up((size_t)n_atoms * sizeof(int32_t), 256);
    const int64_t groups = n_frames < DCV_SUPERPOSE_MAX_GROUPS ? n_frames : DCV_SUPERPOSE_MAX_GROUPS;   // a tile may be one frame
    l.partials = o; o += align_up((size_t)groups * (size_t)n_sel * 6 * sizeof(double), 256);
    l.total = o;
    return l;
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_superpose_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_fit, int32_t n_sel) {
    if (n_frames < 0 || n_atoms <= 0 || n_fit <= 0 || n_sel < 0) return 0;
    return sup_layout(n_frames, n_atoms, n_fit, n_sel).total;
}

extern "C" int dcv_superpose(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                             int32_t n_atoms, const int32_t* fit_h, const double* fit_w_h, const double* fit_ref_h, int32_t n_fit,
                             const int32_t* sel_h, const double* sel_ref_h, int32_t n_sel, double* transform_d, double* rmsd_d,
                             float* aligned_d, int64_t lda, double* moments_d, void* ws_d, size_t ws_bytes, void* stream) {
    // ---- validate everything before anything is launched
    DCV_REQUIRE(xyz_d && fit_h && fit_ref_h && n_frames >= 0 && n_atoms > 0 && n_fit >= 1 && n_sel >= 0,
                "dcv_superpose: bad arguments (n_frames=%lld n_atoms=%d n_fit=%d n_sel=%d)", (long long)n_frames, n_atoms, n_fit, n_sel);
    DCV_REQUIRE_COORD_STRIDES("dcv_superpose", frame_stride, atom_stride, comp_stride);
    DCV_REQUIRE(sel_h || n_sel == 0, "dcv_superpose: n_sel = %d without a selection", n_sel);
    DCV_REQUIRE(!sel_ref_h || n_sel > 0, "dcv_superpose: a selection reference without a selection");
    DCV_REQUIRE(!moments_d || (sel_ref_h && n_sel > 0), "dcv_superpose: moments need a selection and its reference (sel_ref)");
    DCV_REQUIRE(!aligned_d || (n_sel > 0 && lda >= 3 * (int64_t)n_sel), "dcv_superpose: aligned output needs a selection and lda >= 3 n_sel (lda=%lld, n_sel=%d)",
                (long long)lda, n_sel);
    std::vector<char> is_used((size_t)n_atoms, 0);
    for (int32_t i = 0; i < n_fit; ++i) {
        DCV_REQUIRE(fit_h[i] >= 0 && fit_h[i] < n_atoms, "dcv_superpose: fit atom %d is %d, outside [0, %d)", i, fit_h[i], n_atoms);
        is_used[(size_t)fit_h[i]] = 1;
    }
    for (int32_t i = 0; i < n_sel; ++i) {
        DCV_REQUIRE(sel_h[i] >= 0 && sel_h[i] < n_atoms, "dcv_superpose: selected atom %d is %d, outside [0, %d)", i, sel_h[i], n_atoms);
        is_used[(size_t)sel_h[i]] = 1;
    }
    double wsum = 0.0;
    for (int32_t i = 0; i < n_fit; ++i) {
        const double w = fit_w_h ? fit_w_h[i] : 1.0;
        DCV_REQUIRE(std::isfinite(w) && w >= 0.0, "dcv_superpose: weight %d is %g: weights must be finite and >= 0", i, w);
        wsum += w;
    }
    DCV_REQUIRE(wsum > 0.0 && std::isfinite(wsum), "dcv_superpose: the weights sum to %g: the sum must be positive", wsum);
    SupArgs a{};
    StagePlan plan;
    const CoordStrides in{frame_stride, atom_stride, comp_stride};
    stage_plan(is_used, n_atoms, in, a.st, plan);
    const int64_t per_frame = plan.per_frame;
    DCV_REQUIRE_STAGE_FITS("dcv_superpose", per_frame);
    const bool phase_b = aligned_d || moments_d;
    const int64_t xf_bytes = phase_b ? 12 * (int64_t)sizeof(double) : 0;                       // per frame
    const int64_t mom_bytes = moments_d ? (int64_t)n_sel * 6 * (int64_t)sizeof(double) : 0;    // per workgroup
    a.st.tile = stage_tile_frames(per_frame, xf_bytes, mom_bytes);
    const int64_t coord_bytes = (int64_t)align_up((size_t)(a.st.tile * per_frame) * sizeof(float), 16);
    const int64_t lds_bytes = coord_bytes + a.st.tile * xf_bytes + mom_bytes;
    DCV_REQUIRE(lds_bytes <= kStageLdsMax,
                "dcv_superpose: %lld bytes of LDS (one frame of %lld staged atoms%s%s) exceed %d", (long long)lds_bytes, (long long)(per_frame / 3),
                phase_b ? ", its transform" : "", moments_d ? " and 48 bytes of moments per selected atom" : "", kStageLdsMax);
    const SupLayout lay = sup_layout(n_frames, n_atoms, n_fit, n_sel);
    DCV_REQUIRE_WORKSPACE("dcv_superpose", ws_d, ws_bytes, lay.total);
    if (n_frames == 0) return DCV_OK;
    int64_t in_last;
    DCV_REQUIRE_COORDS_FIT("dcv_superpose", coord_extent(n_frames, n_atoms, in, in_last), n_frames, n_atoms);

    // ---- the reference, centred on its weighted centroid, and the LDS slots of both atom lists
    double cr[3] = {0.0, 0.0, 0.0};
    for (int32_t i = 0; i < n_fit; ++i)
        for (int k = 0; k < 3; ++k) cr[k] += (fit_w_h ? fit_w_h[i] : 1.0) * fit_ref_h[3 * (size_t)i + k];
    for (int k = 0; k < 3; ++k) cr[k] /= wsum;
    std::vector<double> rec((size_t)n_fit * 4);
    std::vector<int32_t> fslot((size_t)n_fit), sslot((size_t)n_sel);
    for (int32_t i = 0; i < n_fit; ++i) {
        for (int k = 0; k < 3; ++k) rec[4 * (size_t)i + k] = fit_ref_h[3 * (size_t)i + k] - cr[k];
        rec[4 * (size_t)i + 3] = fit_w_h ? fit_w_h[i] : 1.0;
        fslot[(size_t)i] = plan.slot[(size_t)fit_h[i]];
    }
    for (int32_t i = 0; i < n_sel; ++i) sslot[(size_t)i] = plan.slot[(size_t)sel_h[i]];

    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(ws_d);
    // pageable sources: the runtime has taken its copy of every vector when these calls return
    DCV_CHECK_HIP(hipMemcpyAsync(ws + lay.fit_slot, fslot.data(), fslot.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(ws + lay.fit_rec, rec.data(), rec.size() * sizeof(double), hipMemcpyHostToDevice, s));
    if (n_sel > 0) DCV_CHECK_HIP(hipMemcpyAsync(ws + lay.sel_slot, sslot.data(), sslot.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (sel_ref_h) DCV_CHECK_HIP(hipMemcpyAsync(ws + lay.sel_ref, sel_ref_h, (size_t)n_sel * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(ws + lay.used, plan.used.data(), plan.used.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));

    stage_source(a.st, xyz_d, in, n_frames, reinterpret_cast<const int32_t*>(ws + lay.used));
    a.fit_slot = reinterpret_cast<const int32_t*>(ws + lay.fit_slot);
    a.fit_rec = reinterpret_cast<const double*>(ws + lay.fit_rec);
    a.sel_slot = reinterpret_cast<const int32_t*>(ws + lay.sel_slot);
    a.sel_ref = sel_ref_h ? reinterpret_cast<const double*>(ws + lay.sel_ref) : nullptr;
    a.n_fit = n_fit; a.n_sel = n_sel;
    a.inv_w = 1.0 / wsum;
    for (int k = 0; k < 3; ++k) a.c_ref[k] = cr[k];
    int fl = 1;
    while (fl < kWave && 2 * fl * a.st.tile <= kStageThreads) fl *= 2;   // the lanes of the workgroup dealt to the frames of a tile
    a.fl = fl;
    a.n_tiles = cdiv(n_frames, a.st.tile);
    a.xf_off = (int32_t)coord_bytes;
    a.mom_off = (int32_t)(coord_bytes + a.st.tile * xf_bytes);
    a.transform = transform_d; a.rmsd = rmsd_d; a.aligned = aligned_d; a.lda = lda;
    const int groups = (int)(a.n_tiles < DCV_SUPERPOSE_MAX_GROUPS ? a.n_tiles : DCV_SUPERPOSE_MAX_GROUPS);
    a.partials = moments_d ? reinterpret_cast<double*>(ws + lay.partials) : nullptr;
    hipLaunchKernelGGL(superpose_kernel, dim3((unsigned)groups), dim3(kStageThreads), (size_t)lds_bytes, s, a);
    DCV_CHECK_LAUNCH();
    if (moments_d) {
        const int n = n_sel * 6;
        hipLaunchKernelGGL(superpose_moments_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, a.partials, groups, n, moments_d);
        DCV_CHECK_LAUNCH();
    }
    return DCV_OK;
}

// Featurise and project in one launch (project_trajectory): coordinates in, d <= 16 collective variables out, the
// frames x features matrix never exists in global memory.
//
// A workgroup owns a tile of frames, staged into LDS by stage.h exactly as featurize.hip stages them.  The records are
// walked in PASSES of at most kFpSlab feature values of one class of records, distances or torsions (the host cuts the
// record list, fp_plan).  Per pass:
//   A  lanes along the records, the rest of the workgroup along the frames (as featurize_kernel): the float64 value of
//      feat_math.h, rounded ONCE to float32, normalised in float32 IEEE as dcv_normalize does, stored into the slab
//      xn[frame][value of the pass] in LDS;
//   B  one thread per (frame, slice s): acc[j] += (double)xn * (double)W[.][j] for all D columns (D = d rounded up to 2,
//      4, 8, 16) over the values i = s, s + 16, ... of the pass; xn and the pass's rows of W come from LDS, the D
//      accumulators stay in registers across the passes.
// After the last pass the 16 slices of a frame are added by a butterfly over its 16 lanes and lane j forms
// out_j = (float)((y_j + bias_j - cvmean_j) / cvrange_j) in float64.  The order of the whole sum is therefore a function
// of the record list alone: not of the tile, the grid, the frame count or the layout of the coordinates.
//
// The values of a pass sit in record order ("slots"): a record owns one slot, a sine / cosine record with both features
// two.  A small launch in front gathers W, fmean and frange from feature order into slot order (and pads W to D
// columns with zeros), so the main kernel reads all three linearly; F x D x 4 bytes, L2-resident.
// Per-column extrema: every workgroup leaves its own, minmax.h folds them (as dcv_project_linear).
#include <algorithm>
#include <vector>

#include "common.h"
#include "feat_math.h"
#include "minmax.h"
#include "stage.h"

namespace dcv {

constexpr int kFpThreads = kStageThreads;
constexpr int kFpSlab = 128;                      // feature values per pass
constexpr int kFpSlices = 16;                     // threads per frame in phase B
constexpr int kFpSlabPad = 16;                    // the two frames of a 32-lane group on distinct LDS banks in phase B
constexpr int kFpSlabRow = kFpSlab + kFpSlabPad;  // floats per frame of the slab
constexpr int kFpMaxBlocks = 4096;
constexpr int kFpLdsMax = 160 * 1024;
constexpr int kFpLdsBudget = 52 * 1024;           // three workgroups per CU, which is what 139 - 151 VGPRs (D <= 8) allow too
// device records: kind, four LDS atom slots, first slot of the record, what it stores, 0
constexpr int kFpFirst = 0, kFpSecond = 1, kFpBoth = 2;   // v0 only | v1 only (a lone cosine) | v0 and v1

struct FpArgs {
    StageArgs st;
    const int32_t* recs;    // n_rec x 8
    const int32_t* pass;    // n_pass + 1 pairs: first record, first slot (the last pair: n_rec, F)
    int32_t n_pass;
    int32_t norm;           // gmean / grange are set
    int32_t d;
    double unit;
    const float* gW;        // F x D, slot order
    const float* gmean;     // F, slot order
    const float* grange;
    const float* bias;      // d each, may be null
    const float* cvmean;
    const float* cvrange;
    float* out;
    int64_t ldo;
    float* part;            // [blocks][2][D] or null
    int64_t n_tiles;
};

// W, fmean, frange: feature order -> slot order
__global__ __launch_bounds__(256) void fp_gather_kernel(const int32_t* __restrict__ perm, int F, int d, int D, const float* __restrict__ W,
                                                        const float* __restrict__ fmean, const float* __restrict__ frange,
                                                        float* __restrict__ gW, float* __restrict__ gmean, float* __restrict__ grange) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F * D) return;
    const int slot = i / D, j = i - slot * D, feat = perm[slot];
    gW[i] = j < d ? W[(int64_t)feat * d + j] : 0.f;
    if (j == 0 && fmean) {
        gmean[slot] = fmean[feat];
        grange[slot] = frange[feat];
    }
}

// LDS: slab [tile][kFpSlabRow] | W of the pass [kFpSlab][D] | staged frames [tile][lfs], the first two 16-byte aligned;
// all of it is reused for the extrema at the end of the kernel
template <int D>
__global__ __launch_bounds__(kFpThreads) void featurize_project_kernel(const FpArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* slab = reinterpret_cast<float*>(smem);
    float* Wl = slab + a.st.tile * kFpSlabRow;
    float* lds = Wl + kFpSlab * D;
    const int t = threadIdx.x;
    const int s = t % kFpSlices, fb = t / kFpSlices;   // phase B
    const double unit = a.unit;
    const int las = a.st.las, lcs = a.st.lcs;
    const bool writer = s < a.d;   // lane s of a frame's 16 finishes column s
    const double bias = writer && a.bias ? (double)a.bias[s] : 0.0;
    const double cvmean = writer && a.cvmean ? (double)a.cvmean[s] : 0.0;
    const double cvrange = writer && a.cvrange ? (double)a.cvrange[s] : 1.0;
    float vmin = INFINITY, vmax = -INFINITY;

    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t f0 = tile * a.st.tile;
        const int nf = a.st.n_frames - f0 < a.st.tile ? (int)(a.st.n_frames - f0) : a.st.tile;
        __syncthreads();   // the previous tile has read its frames
        stage_tile(a.st, f0, nf, lds);
        double acc[D];
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] = 0.0;
        for (int p = 0; p < a.n_pass; ++p) {
            const int r0 = a.pass[2 * p], r1 = a.pass[2 * p + 2];
            const int slot0 = a.pass[2 * p + 1], ns = a.pass[2 * p + 3] - slot0;
            __syncthreads();   // the frames are staged; the previous pass has read the slab and its W
            for (int i = t; i < ns * D; i += kFpThreads) Wl[i] = a.gW[(int64_t)slot0 * D + i];
            // phase A: as many lanes along the records as the pass has (a power of two), the rest of the workgroup along the frames
            int dlanes = 1;
            while (dlanes < r1 - r0) dlanes *= 2;
            const int dl = t & (dlanes - 1), fg = t / dlanes, fgroups = kFpThreads / dlanes;
            for (int r = r0 + dl; r < r1; r += dlanes) {
                const int32_t* rec = a.recs + (int64_t)r * 8;
                const int kind = rec[0], s0 = rec[1] * las, s1 = rec[2] * las, s2 = rec[3] * las, s3 = rec[4] * las;
                const int slot = rec[5], what = rec[6];
                float m0 = 0.f, m1 = 0.f, g0 = 1.f, g1 = 1.f;
                if (a.norm) {
                    m0 = a.gmean[slot]; g0 = a.grange[slot];
                    if (what == kFpBoth) { m1 = a.gmean[slot + 1]; g1 = a.grange[slot + 1]; }
                }
                float* x = slab + (slot - slot0);
                for (int f = fg; f < nf; f += fgroups) {
                    const FeatValue v = feature_value(lds + f * a.st.lfs, kind, s0, s1, s2, s3, lcs, unit);
                    float x0 = (float)(what == kFpSecond ? v.v1 : v.v0), x1 = (float)v.v1;
                    if (a.norm) {
                        x0 = __fdiv_rn(__fsub_rn(x0, m0), g0);
                        x1 = __fdiv_rn(__fsub_rn(x1, m1), g1);
                    }
                    x[f * kFpSlabRow] = x0;
                    if (what == kFpBoth) x[f * kFpSlabRow + 1] = x1;
                }
            }
            __syncthreads();
            if (fb < nf) {
                const float* xr = slab + fb * kFpSlabRow;
                for (int i = s; i < ns; i += kFpSlices) {
                    const double x = (double)xr[i];
                    float w[D];
                    if constexpr (D == 2) {
                        const float2 q = *reinterpret_cast<const float2*>(Wl + i * D);
                        w[0] = q.x; w[1] = q.y;
                    } else {
#pragma unroll
                        for (int c = 0; c < D; c += 4) {
                            const float4 q = *reinterpret_cast<const float4*>(Wl + i * D + c);
                            w[c] = q.x; w[c + 1] = q.y; w[c + 2] = q.z; w[c + 3] = q.w;
                        }
                    }
#pragma unroll
                    for (int c = 0; c < D; ++c) acc[c] = fma(x, (double)w[c], acc[c]);   // the product is exact
                }
            }
        }
        // the 16 slices of a frame: a butterfly over its 16 lanes (a + b = b + a: every lane ends with the same bits)
        double y = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            double v = acc[c];
            v += __shfl_xor(v, 8, kWave);
            v += __shfl_xor(v, 4, kWave);
            v += __shfl_xor(v, 2, kWave);
            v += __shfl_xor(v, 1, kWave);
            y = s == c ? v : y;
        }
        if (writer && fb < nf) {
            const float o = (float)((y + bias - cvmean) / cvrange);
            a.out[(f0 + fb) * a.ldo + s] = o;
            vmin = fminf(vmin, o);
            vmax = fmaxf(vmax, o);
        }
    }
    if (a.part) {
        __syncthreads();
        float* red = reinterpret_cast<float*>(smem);   // [2][D][16 frames]
        if (s < D) {
            red[(0 * D + s) * 16 + fb] = vmin;
            red[(1 * D + s) * 16 + fb] = vmax;
        }
        __syncthreads();
        if (t < 2 * D) {
            const int which = t / D, c = t % D;
            float v = which == 0 ? INFINITY : -INFINITY;
            for (int q = 0; q < 16; ++q) {
                const float w = red[(which * D + c) * 16 + q];
                v = which == 0 ? fminf(v, w) : fmaxf(v, w);
            }
            a.part[((int64_t)blockIdx.x * 2 + which) * D + c] = v;
        }
    }
}

// The cut of the record list into passes of at most kFpSlab values of one class of records (distances | torsions), and
// the slot of every record: a function of the records alone.  what[r]: kFpFirst / kFpSecond / kFpBoth.
struct FpPlan {
    std::vector<int32_t> slot, what, pass, perm;   // per record | per record | n_pass + 1 pairs (record, slot) | feature of every slot
};

static void fp_plan(const int32_t* rec_h, int32_t n_rec, FpPlan& p) {
    p.slot.resize((size_t)n_rec);
    p.what.resize((size_t)n_rec);
    p.pass.assign(2, 0);
    p.perm.clear();
    int32_t in_pass = 0;
    bool torsions = false;   // a pass holds distances or torsions, not both: its lanes then do the same work
    for (int32_t r = 0; r < n_rec; ++r) {
        const int32_t* q = rec_h + (size_t)r * 8;
        const int32_t what = q[5] >= 0 && q[6] >= 0 ? kFpBoth : (q[5] >= 0 ? kFpFirst : kFpSecond);
        const int32_t n = what == kFpBoth ? 2 : 1;
        const bool torsion = q[0] != DCV_FEAT_DISTANCE;
        if (in_pass == 0) torsions = torsion;
        if (in_pass + n > kFpSlab || torsion != torsions) {
            p.pass.push_back(r);
            p.pass.push_back((int32_t)p.perm.size());
            in_pass = 0;
            torsions = torsion;
        }
        in_pass += n;
        p.slot[(size_t)r] = (int32_t)p.perm.size();
        p.what[(size_t)r] = what;
        if (q[5] >= 0) p.perm.push_back(q[5]);
        if (q[6] >= 0) p.perm.push_back(q[6]);
    }
    p.pass.push_back(n_rec);
    p.pass.push_back((int32_t)p.perm.size());
}

// workspace: records | used atoms | passes | perm | gW | gmean | grange | part
struct FpWorkspace {
    size_t recs, used, pass, perm, gW, gmean, grange, part, total;
};

static FpWorkspace fp_workspace(int32_t n_atoms, int32_t n_rec, int32_t F) {
    FpWorkspace w{};
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += align_up(bytes, 256);
        return at;
    };
    w.recs = take((size_t)n_rec * 8 * sizeof(int32_t));
    w.used = take((size_t)n_atoms * sizeof(int32_t));
    w.pass = take(((size_t)n_rec + 1) * 2 * sizeof(int32_t));
    w.perm = take((size_t)F * sizeof(int32_t));
    w.gW = take((size_t)F * 16 * sizeof(float));
    w.gmean = take((size_t)F * sizeof(float));
    w.grange = take((size_t)F * sizeof(float));
    w.part = take((size_t)kFpMaxBlocks * 2 * 16 * sizeof(float));
    w.total = o;
    return w;
}

template <int D>
static int launch_featurize_project(const FpArgs& a, int blocks, size_t lds, float* minmax, hipStream_t s) {
    if (lds > 64 * 1024)
        DCV_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&featurize_project_kernel<D>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((featurize_project_kernel<D>), dim3((unsigned)blocks), dim3(kFpThreads), lds, s, a);
    DCV_CHECK_LAUNCH();
    if (minmax) {
        hipLaunchKernelGGL(project_minmax_final<D>, dim3(2 * a.d), dim3(256), 0, s, a.part, blocks, a.d, minmax);
        DCV_CHECK_LAUNCH();
    }
    return DCV_OK;
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_featurize_project_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_rec, int32_t F, int32_t d) {
    if (n_frames < 0 || n_atoms <= 0 || n_rec <= 0 || F <= 0 || d < 1 || d > 16) return 0;
    return fp_workspace(n_atoms, n_rec, F).total;
}

extern "C" int dcv_featurize_project(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                                     int32_t n_atoms, const int32_t* rec_h, int32_t n_rec, int32_t F, double unit, const float* fmean_d,
                                     const float* frange_d, const float* W_d, int32_t d, const float* bias_d, const float* cvmean_d,
                                     const float* cvrange_d, float* out_d, int64_t ldo, float* minmax_d, void* ws_d, size_t ws_bytes,
                                     void* stream) {
    DCV_REQUIRE(xyz_d && rec_h && W_d && out_d && n_frames >= 0 && n_atoms > 0 && n_rec > 0 && F > 0,
                "dcv_featurize_project: bad arguments (n_frames=%lld n_atoms=%d n_rec=%d F=%d)", (long long)n_frames, n_atoms, n_rec, F);
    DCV_REQUIRE(d >= 1 && d <= 16, "dcv_featurize_project: d=%d unsupported (1..16)", d);
    DCV_REQUIRE(ldo >= d, "dcv_featurize_project: ldo = %lld is smaller than d = %d", (long long)ldo, d);
    DCV_REQUIRE((fmean_d == nullptr) == (frange_d == nullptr), "dcv_featurize_project: fmean/frange must come together");
    DCV_REQUIRE((cvmean_d == nullptr) == (cvrange_d == nullptr), "dcv_featurize_project: cvmean/cvrange must come together");
    DCV_REQUIRE_COORD_STRIDES("dcv_featurize_project", frame_stride, atom_stride, comp_stride);
    // ---- validate every record before anything is launched
    std::vector<char> is_used((size_t)n_atoms, 0);
    std::vector<int32_t> writers((size_t)F, 0);
    for (int32_t r = 0; r < n_rec; ++r) {
        const int32_t* q = rec_h + (size_t)r * 8;
        const int32_t kind = q[0];
        DCV_REQUIRE(kind == DCV_FEAT_DISTANCE || kind == DCV_FEAT_TORSION_SINCOS || kind == DCV_FEAT_TORSION,
                    "dcv_featurize_project: record %d has unknown kind %d", r, kind);
        const int na = kind == DCV_FEAT_DISTANCE ? 2 : 4;
        for (int k = 0; k < na; ++k) {
            DCV_REQUIRE(q[1 + k] >= 0 && q[1 + k] < n_atoms, "dcv_featurize_project: record %d names atom %d, outside [0, %d)", r, q[1 + k],
                        n_atoms);
            is_used[(size_t)q[1 + k]] = 1;
        }
        DCV_REQUIRE(q[5] >= -1 && q[5] < F && q[6] >= -1 && q[6] < F && (q[5] >= 0 || q[6] >= 0),
                    "dcv_featurize_project: record %d names features (%d, %d): each in [-1, %d), at least one >= 0", r, q[5], q[6], F);
        DCV_REQUIRE(kind == DCV_FEAT_TORSION_SINCOS || (q[5] >= 0 && q[6] == -1),
                    "dcv_featurize_project: record %d of kind %d has one value, its features are (%d, %d)", r, kind, q[5], q[6]);
        if (q[5] >= 0) ++writers[(size_t)q[5]];
        if (q[6] >= 0) ++writers[(size_t)q[6]];
    }
    for (int32_t i = 0; i < F; ++i)
        DCV_REQUIRE(writers[(size_t)i] == 1, "dcv_featurize_project: feature %d is written by %d records, every feature needs exactly one", i,
                    writers[(size_t)i]);

    FpArgs a{};
    StagePlan plan;
    const CoordStrides in{frame_stride, atom_stride, comp_stride};
    stage_plan(is_used, n_atoms, in, a.st, plan);
    DCV_REQUIRE_STAGE_FITS("dcv_featurize_project", plan.per_frame);
    const FpWorkspace w = fp_workspace(n_atoms, n_rec, F);
    DCV_REQUIRE_WORKSPACE("dcv_featurize_project", ws_d, ws_bytes, w.total);
    if (n_frames == 0) return DCV_OK;
    int64_t in_last;
    DCV_REQUIRE_COORDS_FIT("dcv_featurize_project", coord_extent(n_frames, n_atoms, in, in_last), n_frames, n_atoms);

    const int D = d <= 2 ? 2 : d <= 4 ? 4 : d <= 8 ? 8 : 16;
    const int64_t fixed = (int64_t)kFpSlab * D * sizeof(float), per = (plan.per_frame + kFpSlabRow) * (int64_t)sizeof(float);
    a.st.tile = (int)std::min<int64_t>(kStageTile, std::max<int64_t>(1, (kFpLdsBudget - fixed) / per));
    if (a.st.tile > 4) a.st.tile &= ~3;   // a pass of 64 sine / cosine records splits the frames over 4 groups of threads: no ragged group
    const size_t lds = std::max((size_t)(a.st.tile * per + fixed), (size_t)2 * 16 * 16 * sizeof(float));
    DCV_REQUIRE(lds <= (size_t)kFpLdsMax, "dcv_featurize_project: %zu bytes of LDS (max %d)", lds, kFpLdsMax);
    a.n_tiles = cdiv(n_frames, a.st.tile);
    int64_t blocks = a.n_tiles;
    if (blocks > (int64_t)num_cus() * 8) blocks = (int64_t)num_cus() * 8;
    if (blocks > kFpMaxBlocks) blocks = kFpMaxBlocks;

    // ---- the records with atoms as LDS slots, their passes, the feature of every slot
    FpPlan fp;
    fp_plan(rec_h, n_rec, fp);
    std::vector<int32_t> rec((size_t)n_rec * 8, 0);
    for (int32_t r = 0; r < n_rec; ++r) {
        const int32_t* q = rec_h + (size_t)r * 8;
        int32_t* o = rec.data() + (size_t)r * 8;
        const int na = q[0] == DCV_FEAT_DISTANCE ? 2 : 4;
        o[0] = q[0];
        for (int k = 0; k < na; ++k) o[1 + k] = plan.slot[(size_t)q[1 + k]];
        o[5] = fp.slot[(size_t)r];
        o[6] = fp.what[(size_t)r];
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(ws_d);
    int32_t* perm_d = reinterpret_cast<int32_t*>(ws + w.perm);
    // pageable sources: the runtime has taken its copy of the vectors when these calls return
    DCV_CHECK_HIP(hipMemcpyAsync(ws + w.recs, rec.data(), rec.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(ws + w.used, plan.used.data(), plan.used.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(ws + w.pass, fp.pass.data(), fp.pass.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(perm_d, fp.perm.data(), fp.perm.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));

    float* gW = reinterpret_cast<float*>(ws + w.gW);
    float* gmean = reinterpret_cast<float*>(ws + w.gmean);
    float* grange = reinterpret_cast<float*>(ws + w.grange);
    hipLaunchKernelGGL(fp_gather_kernel, dim3((unsigned)cdiv((int64_t)F * D, 256)), dim3(256), 0, s, perm_d, F, d, D, W_d, fmean_d, frange_d, gW,
                       gmean, grange);
    DCV_CHECK_LAUNCH();

    stage_source(a.st, xyz_d, in, n_frames, reinterpret_cast<const int32_t*>(ws + w.used));
    a.recs = reinterpret_cast<const int32_t*>(ws + w.recs);
    a.pass = reinterpret_cast<const int32_t*>(ws + w.pass);
    a.n_pass = (int32_t)fp.pass.size() / 2 - 1;
    a.norm = fmean_d != nullptr;
    a.d = d;
    a.unit = unit;
    a.gW = gW; a.gmean = gmean; a.grange = grange;
    a.bias = bias_d; a.cvmean = cvmean_d; a.cvrange = cvrange_d;
    a.out = out_d; a.ldo = ldo;
    a.part = minmax_d ? reinterpret_cast<float*>(ws + w.part) : nullptr;
    if (D == 2) return launch_featurize_project<2>(a, (int)blocks, lds, minmax_d, s);
    if (D == 4) return launch_featurize_project<4>(a, (int)blocks, lds, minmax_d, s);
    if (D == 8) return launch_featurize_project<8>(a, (int)blocks, lds, minmax_d, s);
    return launch_featurize_project<16>(a, (int)blocks, lds, minmax_d, s);
}

// Featurisation (compute_features): distances and torsions from trajectory coordinates, frames x atoms x 3 float32 in,
// frames x features float32 out.
//
// A workgroup owns a tile of kStageTile frames (fewer when the atoms it needs do not fit the LDS budget).  It stages
// the coordinates of the atoms the features use into LDS with coalesced loads, computes every feature of its frames
// in float64 from LDS (feat_math.h: PLUMED computes in double, p = (double)x * unit; one rounding to float32 on store)
// and writes the output rows with consecutive lanes on consecutive columns.  No atomics, no state between workgroups.
//
// The two staging forms (ROWS and GATHER), their host-side choice and the LDS budget live in stage.h, which
// superpose.hip shares.
#include <algorithm>
#include <vector>

#include "common.h"
#include "feat_math.h"
#include "stage.h"

namespace dcv {

constexpr int kFeatThreads = kStageThreads;

struct FeatArgs {
    StageArgs st;
    const int32_t* defs;   // n_defs x 6: kind, four atom indices REMAPPED to LDS atom slots, output column
    int32_t n_defs;
    double unit;
    float* out;
    int64_t ldo;
};

__global__ __launch_bounds__(kFeatThreads) void featurize_kernel(const FeatArgs a, const int dlanes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* lds = reinterpret_cast<float*>(smem);
    const int64_t f0 = (int64_t)blockIdx.x * a.st.tile;
    const int nf = a.st.n_frames - f0 < a.st.tile ? (int)(a.st.n_frames - f0) : a.st.tile;
    stage_tile(a.st, f0, nf, lds);
    __syncthreads();

    // lanes along the definitions (consecutive lanes -> consecutive output columns), the rest of the workgroup along frames
    const int t = threadIdx.x;
    const int dl = t & (dlanes - 1), fg = t / dlanes, fgroups = kFeatThreads / dlanes;
    const double unit = a.unit;
    const int las = a.st.las, lcs = a.st.lcs;
    for (int d = dl; d < a.n_defs; d += dlanes) {
        const int32_t* rec = a.defs + (int64_t)d * 6;
        const int kind = rec[0], s0 = rec[1] * las, s1 = rec[2] * las, s2 = rec[3] * las, s3 = rec[4] * las;
        float* o = a.out + rec[5];
        for (int f = fg; f < nf; f += fgroups) {
            const float* lf = lds + f * a.st.lfs;
            float* of = o + (f0 + f) * a.ldo;
            const FeatValue v = feature_value(lf, kind, s0, s1, s2, s3, lcs, unit);
            of[0] = (float)v.v0;
            if (kind == DCV_FEAT_TORSION_SINCOS) of[1] = (float)v.v1;
        }
    }
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_featurize_workspace(int64_t n_frames, int32_t n_atoms, int32_t n_defs) {
    if (n_frames < 0 || n_atoms <= 0 || n_defs <= 0) return 0;
    return align_up((size_t)n_defs * 6 * sizeof(int32_t), 256) + align_up((size_t)n_atoms * sizeof(int32_t), 256);
}

extern "C" int dcv_featurize(const float* xyz_d, int64_t n_frames, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                             int32_t n_atoms, const int32_t* defs_h, int32_t n_defs, double unit, float* out_d, int64_t ldo,
                             void* ws_d, size_t ws_bytes, void* stream) {
    DCV_REQUIRE(xyz_d && defs_h && out_d && n_frames >= 0 && n_atoms > 0 && n_defs > 0 && ldo > 0,
                "dcv_featurize: bad arguments (n_frames=%lld n_atoms=%d n_defs=%d ldo=%lld)", (long long)n_frames, n_atoms, n_defs,
                (long long)ldo);
    DCV_REQUIRE_COORD_STRIDES("dcv_featurize", frame_stride, atom_stride, comp_stride);
    // ---- validate every record before anything is launched
    std::vector<char> is_used((size_t)n_atoms, 0);
    for (int32_t d = 0; d < n_defs; ++d) {
        const int32_t* r = defs_h + (size_t)d * 6;
        const int32_t kind = r[0];
        DCV_REQUIRE(kind == DCV_FEAT_DISTANCE || kind == DCV_FEAT_TORSION_SINCOS || kind == DCV_FEAT_TORSION,
                    "dcv_featurize: record %d has unknown kind %d", d, kind);
        const int na = kind == DCV_FEAT_DISTANCE ? 2 : 4, nc = kind == DCV_FEAT_TORSION_SINCOS ? 2 : 1;
        for (int k = 0; k < na; ++k) {
            DCV_REQUIRE(r[1 + k] >= 0 && r[1 + k] < n_atoms, "dcv_featurize: record %d names atom %d, outside [0, %d)", d, r[1 + k], n_atoms);
            is_used[(size_t)r[1 + k]] = 1;
        }
        DCV_REQUIRE(r[5] >= 0 && (int64_t)r[5] + nc <= ldo, "dcv_featurize: record %d writes column %d (+%d), outside ldo = %lld", d, r[5],
                    nc - 1, (long long)ldo);
    }
    DCV_REQUIRE_WORKSPACE("dcv_featurize", ws_d, ws_bytes, dcv_featurize_workspace(n_frames, n_atoms, n_defs));
    if (n_frames == 0) return DCV_OK;
    const CoordStrides in{frame_stride, atom_stride, comp_stride};
    int64_t in_last;
    DCV_REQUIRE_COORDS_FIT("dcv_featurize", coord_extent(n_frames, n_atoms, in, in_last), n_frames, n_atoms);

    // ---- the atoms to stage and their LDS slots
    FeatArgs a{};
    StagePlan plan;
    stage_plan(is_used, n_atoms, in, a.st, plan);
    const std::vector<int32_t>&used = plan.used, &slot = plan.slot;
    const int64_t per_frame = plan.per_frame;
    DCV_REQUIRE_STAGE_FITS("dcv_featurize", per_frame);
    a.st.tile = stage_tile_frames(per_frame, 0, 0);
    const int64_t blocks = cdiv(n_frames, a.st.tile);
    DCV_REQUIRE(blocks <= 0x7fffffffLL, "dcv_featurize: %lld frames need more than 2^31 - 1 workgroups", (long long)n_frames);

    std::vector<int32_t> rec((size_t)n_defs * 6, 0);
    for (int32_t d = 0; d < n_defs; ++d) {
        const int32_t* r = defs_h + (size_t)d * 6;
        int32_t* w = rec.data() + (size_t)d * 6;
        const int na = r[0] == DCV_FEAT_DISTANCE ? 2 : 4;
        w[0] = r[0];
        for (int k = 0; k < na; ++k) w[1 + k] = slot[(size_t)r[1 + k]];
        w[5] = r[5];
    }
    hipStream_t s = as_stream(stream);
    int32_t* defs_d = static_cast<int32_t*>(ws_d);
    int32_t* used_d = reinterpret_cast<int32_t*>(static_cast<char*>(ws_d) + align_up((size_t)n_defs * 6 * sizeof(int32_t), 256));
    // pageable sources: the runtime has taken its copy of both vectors when these calls return
    DCV_CHECK_HIP(hipMemcpyAsync(defs_d, rec.data(), rec.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipMemcpyAsync(used_d, used.data(), used.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));

    stage_source(a.st, xyz_d, in, n_frames, used_d);
    a.defs = defs_d;
    a.n_defs = n_defs;
    a.unit = unit;
    a.out = out_d; a.ldo = ldo;
    int dlanes = 1;
    while (dlanes < kFeatThreads && dlanes < n_defs) dlanes *= 2;
    const size_t lds = (size_t)a.st.tile * (size_t)per_frame * sizeof(float);
    hipLaunchKernelGGL(featurize_kernel, dim3((unsigned)blocks), dim3(kFeatThreads), lds, s, a, dlanes);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

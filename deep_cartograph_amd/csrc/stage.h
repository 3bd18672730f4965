// Staging of trajectory coordinates into LDS, shared by the kernels that stream frames (featurize.hip, superpose.hip).
//
// A workgroup of kStageThreads threads owns a tile of frames (kStageTile, fewer when the atoms it needs do not fit the
// LDS budget) and copies the coordinates of the atoms it uses into LDS with coalesced loads.  Two forms, chosen on the
// host (stage_plan) from the strides and the set of atoms used:
//   ROWS    the innermost stride is 1 (dense (n, A, 3) rows, or the X / Y / Z planes of a DCD frame record) and the
//           used atoms fill at least half of their index range [a_lo, a_hi]: that whole range is copied as contiguous
//           rows with 16-byte loads on the 16-byte grid of the ADDRESS (the rows of a DCD record start anywhere), the
//           ragged head and tail of a row with guarded scalar loads;
//   GATHER  everything else (any strides, a sparse subset of an all-atom trajectory): one 4-byte load per coordinate
//           of a used atom, lanes along the sorted list of used atoms, nothing else is read.
// In LDS, coordinate c of the atom in slot s of frame f of the tile is lds[f * lfs + s * las + c * lcs].
// The 16-byte load is stream.h's; strides, layout forms and the stride requirement are coords.h's.  The host preamble of
// the staging entries is at the end: the refusal of a frame that LDS cannot hold and the source fields of StageArgs.
#pragma once
#include <vector>

#include "coords.h"
#include "stream.h"

namespace dcv {

constexpr int kStageThreads = 256;
constexpr int kStageTile = 16;               // frames per workgroup
constexpr int kStageLdsBudget = 48 * 1024;   // three workgroups per CU
constexpr int kStageLdsMax = 64 * 1024;      // one frame of the needed atoms must fit: 5461 atoms

struct StageArgs {
    const float* xyz;
    CoordStrides in;
    int64_t n_frames;
    const int32_t* used;   // GATHER: the nu used atoms, ascending
    int32_t nu;
    int32_t rows;          // 1 = ROWS staging, 0 = GATHER
    int32_t rpf;           // ROWS: rows per frame (3 planes, or 1 dense row)
    int32_t L;             // ROWS: floats per row
    int64_t row_off;       // ROWS: a_lo * atom_stride
    int32_t comp_fast;     // GATHER: the component runs fastest over the lanes (coord_comp_fast)
    int32_t lfs, las, lcs; // LDS strides of frame, atom slot, component
    int32_t tile;          // frames per workgroup
};

// Contiguous rows -> LDS.  A slot is one 16-byte-aligned group of four floats of the address space; slot k of a row
// that starts m floats past such a boundary holds row elements 4k - m .. 4k - m + 3.  Four slots per thread are in
// flight before the first LDS store.
__device__ __forceinline__ void stage_rows(const StageArgs& a, int64_t f0, int nf, float* lds) {
    const int t = threadIdx.x;
    const int nsmax = (a.L + 6) >> 2;   // slots of a row for the worst alignment
    const int total = nf * a.rpf * nsmax;
    constexpr int U = 4;
    for (int base = t; base < total; base += kStageThreads * U) {
        float4 v[U];
        const float* g[U];
        float* l[U];
        int j0[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * kStageThreads;
            j0[u] = INT32_MIN;
            if (i >= total) continue;
            const int row = i / nsmax, k = i - row * nsmax;
            const int f = row / a.rpf, c = row - f * a.rpf;
            g[u] = a.xyz + (f0 + f) * a.in.f + (int64_t)c * a.in.c + a.row_off;
            l[u] = lds + row * a.L;
            const int m = (int)((reinterpret_cast<uintptr_t>(g[u]) >> 2) & 3);
            const int j = 4 * k - m;
            if (j >= a.L) continue;   // this row has fewer slots than nsmax
            j0[u] = j;
            if (j >= 0 && j + 4 <= a.L) v[u] = nt_load4(g[u] + j);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0[u];
            if (j == INT32_MIN) continue;
            if (j >= 0 && j + 4 <= a.L) {
                l[u][j] = v[u].x; l[u][j + 1] = v[u].y; l[u][j + 2] = v[u].z; l[u][j + 3] = v[u].w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (j + e >= 0 && j + e < a.L) l[u][j + e] = g[u][j + e];
            }
        }
    }
}

// Used atoms only -> LDS laid out [frame][component][slot].
__device__ __forceinline__ void stage_gather(const StageArgs& a, int64_t f0, int nf, float* lds) {
    const int per = 3 * a.nu;
    const int total = nf * per;
    for (int i = threadIdx.x; i < total; i += kStageThreads) {
        const int f = i / per, r = i - f * per;
        int c, u;
        if (a.comp_fast) { u = r / 3; c = r - u * 3; }
        else { c = r / a.nu; u = r - c * a.nu; }
        const int64_t off = (f0 + f) * a.in.f + (int64_t)a.used[u] * a.in.a + (int64_t)c * a.in.c;
        lds[f * per + c * a.nu + u] = a.xyz[off];
    }
}

__device__ __forceinline__ void stage_tile(const StageArgs& a, int64_t f0, int nf, float* lds) {
    if (a.rows) stage_rows(a, f0, nf, lds);
    else stage_gather(a, f0, nf, lds);
}

// Host side: the atoms to stage (ascending), the LDS slot of every atom and the staging form.
struct StagePlan {
    std::vector<int32_t> used, slot;
    int64_t per_frame = 0;   // LDS floats per frame
};

// Fills the staging fields of `a` (everything but xyz / strides / n_frames / used / tile) and `p` from the flags
// is_used[n_atoms] (at least one set).  The caller checks per_frame against the LDS it has and picks the tile.
inline void stage_plan(const std::vector<char>& is_used, int32_t n_atoms, const CoordStrides& in, StageArgs& a, StagePlan& p) {
    p.used.clear();
    p.slot.assign((size_t)n_atoms, 0);
    for (int32_t i = 0; i < n_atoms; ++i)
        if (is_used[(size_t)i]) p.used.push_back(i);
    const int32_t nu = (int32_t)p.used.size(), a_lo = p.used.front(), a_hi = p.used.back();
    const int64_t range = (int64_t)a_hi - a_lo + 1;
    const bool planes = coord_form(in) == kCoordPlanes;
    a.nu = nu;
    a.rows = coord_form(in) != kCoordStrided && range <= 2 * (int64_t)nu;
    if (a.rows) {
        for (int32_t i = a_lo; i <= a_hi; ++i) p.slot[(size_t)i] = i - a_lo;
        p.per_frame = 3 * range;
        a.rpf = planes ? 3 : 1;
        a.L = (int32_t)(planes ? range : 3 * range);
        a.row_off = (int64_t)a_lo * in.a;
        a.las = planes ? 1 : 3;
        a.lcs = planes ? (int32_t)range : 1;
    } else {
        for (int32_t u = 0; u < nu; ++u) p.slot[(size_t)p.used[(size_t)u]] = u;
        p.per_frame = 3 * (int64_t)nu;
        a.comp_fast = coord_comp_fast(in);
        a.las = 1;
        a.lcs = nu;
    }
    a.lfs = (int32_t)p.per_frame;
}

// Frames per workgroup when `fixed_bytes` of LDS are taken by something else: as many as fit the budget, 1 .. kStageTile.
inline int stage_tile_frames(int64_t per_frame, int64_t bytes_per_frame_extra, int64_t fixed_bytes) {
    const int64_t per = per_frame * (int64_t)sizeof(float) + bytes_per_frame_extra;
    const int64_t tile = (kStageLdsBudget - fixed_bytes) / per;
    return tile < 1 ? 1 : (tile > kStageTile ? kStageTile : (int)tile);
}

// where the coordinates come from: everything of `a` that stage_plan and the choice of the tile leave open
inline void stage_source(StageArgs& a, const float* xyz, const CoordStrides& in, int64_t n_frames, const int32_t* used_d) {
    a.xyz = xyz;
    a.in = in;
    a.n_frames = n_frames;
    a.used = used_d;
}

// one frame of the staged atoms (StagePlan::per_frame floats) must fit the LDS of a workgroup
#define DCV_REQUIRE_STAGE_FITS(entry, per_frame)                                                                                  \
    DCV_REQUIRE((per_frame) * (int64_t)sizeof(float) <= dcv::kStageLdsMax,                                                        \
                entry ": one frame of the %lld atoms to stage exceeds %d bytes of LDS (at most %d atoms)", (long long)((per_frame) / 3), \
                dcv::kStageLdsMax, dcv::kStageLdsMax / 12)

}  // namespace dcv

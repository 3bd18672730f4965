// The finishing launch of per-column extrema, shared by the kernels that project frames (project.hip,
// featurize_project.hip): every workgroup of the projecting launch leaves part[block][min | max][D], this launch folds
// the blocks.  min / max are exact in any order, so the result does not depend on the grid.
#pragma once
#include "common.h"

namespace dcv {

// one workgroup per (min | max, component): threads take the blocks b = t, t + 256, ..., LDS tree
template <int D>
__global__ __launch_bounds__(256) void project_minmax_final(const float* __restrict__ part, int nblocks, int d, float* __restrict__ minmax) {
    __shared__ float s_red[256];
    const int t = threadIdx.x;
    const int which = blockIdx.x / d, c = blockIdx.x % d;
    float v = which == 0 ? INFINITY : -INFINITY;
    for (int b = t; b < nblocks; b += 256) {
        const float w = part[((int64_t)b * 2 + which) * D + c];
        v = which == 0 ? fminf(v, w) : fmaxf(v, w);
    }
    s_red[t] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) s_red[t] = which == 0 ? fminf(s_red[t], s_red[t + o]) : fmaxf(s_red[t], s_red[t + o]);
        __syncthreads();
    }
    if (t == 0) minmax[which * d + c] = s_red[0];
}

}  // namespace dcv

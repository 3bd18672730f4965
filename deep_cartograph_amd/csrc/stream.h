// Shared pieces of the float32 streaming passes (stats.hip, filter.hip, project.hip, stage.h), ONE copy each: the
// non-temporal 16-byte access, the load of one column group and the walk over a block's rows with U loads in flight.
// The block's rows (block_rows) and the host's rule for 16-byte accesses (quad_path / quad_ok / aligned16) are in common.h.
#pragma once
#include "common.h"

namespace dcv {

// 16-byte non-temporal accesses: the matrix is streamed once per pass (round 4: the same policy took the k-means point
// stream from 4.6 to 5.7 TB/s, the normalisation +2.7 %)
typedef float nt_float4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 nt_load4(const float* p) {
    const nt_float4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_float4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void nt_store4(float* p, const float4& v) {   // by value costs normalize_rows_kernel two VGPRs
    __builtin_nontemporal_store(nt_float4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_float4*>(p));
}

// one column group: VEC = 4 a non-temporal 16-byte load (the host took quad_path), VEC = 1 a plain scalar load
template <int VEC>
__device__ __forceinline__ void load_group(const float* p, float (&x)[VEC]) {
    static_assert(VEC == 1 || VEC == 4, "a column group is one float or four");
    if constexpr (VEC == 4) {
        const float4 q = nt_load4(p);
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        x[0] = *p;
    }
}

// Rows r, r + step, ... < r_end of the column group at `base` (row stride ld): f(value, v) for every value, v < VEC its
// place in the group.  U independent row loads are in flight before the first value is used; the tail takes a row at a time.
template <int VEC, int U, class F>
__device__ __forceinline__ void stream_rows(const float* base, int64_t ld, int64_t r, int64_t r_end, int64_t step, F&& f) {
    for (; r + (U - 1) * step < r_end; r += U * step) {
        float x[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) load_group<VEC>(base + (r + u * step) * ld, x[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int v = 0; v < VEC; ++v) f(x[u][v], v);
    }
    for (; r < r_end; r += step) {
        float x[VEC];
        load_group<VEC>(base + r * ld, x);
#pragma unroll
        for (int v = 0; v < VEC; ++v) f(x[v], v);
    }
}

}  // namespace dcv

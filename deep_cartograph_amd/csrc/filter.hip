// Feature filtering (filter_features): per-column histograms with NumPy's bin semantics and Hartigan's dip
// statistic of sorted columns.
//
// Histogram: one streaming pass over the frames x features matrix.  Lanes run along the feature axis (16-byte
// loads), a workgroup owns a block of kHistCols columns and a contiguous range of rows, counts into an LDS
// histogram per column with LDS atomics and adds its non-zero counters to the int64 result with NON-returning
// global atomics (integer sums do not depend on the order, so the result is deterministic).
//
// Dip: one lane per column, columns adjacent in memory (n x C row-major), float64 arithmetic on the float32
// values, no fused multiply-adds, so the statistic is the one a float64 host implementation of AS 217 gives.
// The hull scans keep the top of each lane's vertex stack in LDS.
// The histogram's loads, its walk over a block's rows and the rule for 16-byte accesses are stream.h's.
#include "stream.h"

namespace dcv {

constexpr int kHistThreads = 256;
constexpr int kHistCols = 64;      // columns per workgroup: 64 x (bins + 1) counters and edges in LDS (51.7 KB at 100 bins)
constexpr int kHistMaxBins = 126;  // 64 columns x 127 x 8 bytes = 63.5 KB of LDS

// odd, so never a multiple of the 32 banks: the columns of a wave start in different banks
__host__ __device__ inline int hist_stride(int bins) { return (bins + 1) | 1; }

template <int VEC>
__global__ __launch_bounds__(kHistThreads) void col_histogram_kernel(const float* __restrict__ X, int64_t n, int F, int64_t ld,
                                                                     const float* __restrict__ edges, int bins,
                                                                     unsigned long long* __restrict__ counts,
                                                                     int64_t rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int stride = hist_stride(bins);
    unsigned int* s_cnt = reinterpret_cast<unsigned int*>(smem);        // [kHistCols][stride]
    float* s_edge = reinterpret_cast<float*>(s_cnt + kHistCols * stride);  // [kHistCols][stride]
    const int t = threadIdx.x;
    const int c0 = blockIdx.y * kHistCols;
    const int nc = F - c0 < kHistCols ? F - c0 : kHistCols;
    for (int i = t; i < kHistCols * stride; i += kHistThreads) s_cnt[i] = 0u;
    for (int i = t; i < nc * (bins + 1); i += kHistThreads) {
        const int c = i / (bins + 1), b = i - c * (bins + 1);
        s_edge[c * stride + b] = edges[(int64_t)(c0 + c) * (bins + 1) + b];
    }
    __syncthreads();

    constexpr int G = kHistCols / VEC;       // column groups
    constexpr int RL = kHistThreads / G;     // row lanes
    const int cg = t % G, rl = t / G;
    const int col = cg * VEC;
    const Range rows = block_rows(n, rows_per_block);
    if (col < nc) {
        float first[VEC], last[VEC], scale[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            first[v] = s_edge[(col + v) * stride];
            last[v] = s_edge[(col + v) * stride + bins];
            scale[v] = (float)bins / (last[v] - first[v]);
        }
        auto count = [&](float x, int v) {
            if (!(x >= first[v] && x <= last[v])) return;   // np.histogram drops what lies outside the range
            const float* e = s_edge + (col + v) * stride;
            int i = (int)((x - first[v]) * scale[v]);        // guessed bin, corrected against the edges below
            i = i < 0 ? 0 : (i > bins - 1 ? bins - 1 : i);
            while (i > 0 && x < e[i]) --i;
            while (i < bins - 1 && x >= e[i + 1]) ++i;        // the last bin is closed on the right
            atomicAdd(&s_cnt[(col + v) * stride + i], 1u);
        };
        stream_rows<VEC, 4>(X + c0 + col, ld, rows.begin + rl, rows.end, RL, count);   // 4 independent row loads in flight
    }
    __syncthreads();
    for (int i = t; i < nc * bins; i += kHistThreads) {
        const int c = i / bins, b = i - c * bins;
        const unsigned int k = s_cnt[c * stride + b];
        if (k) atomicAdd(&counts[(int64_t)(c0 + c) * bins + b], (unsigned long long)k);   // result unused: no return
    }
}

// ------------------------------------------------------------------------------------------------ dip statistic
// Hartigan & Hartigan 1985, AS 217, with Maechler's termination test and the symmetric dx formula.  Indices are
// 1-based as in the published algorithm; element j of column c of a work array lives at [j * C + c], so the lanes
// of a wave (consecutive columns) touch consecutive words whenever they are at the same j.
constexpr int kDipWindow = 32;   // hull vertices per lane kept in LDS: 32 x 8 bytes x 64 lanes = 16 KB per wave
constexpr int kDipBatch = 8;     // rows of the column per batch of the hull scans (one batch is requested ahead)
constexpr int kDipDeep = 32;     // independent loads in flight in the scans between hull vertices

// One hull scan: FWD builds the greatest convex minorant links mn[j] (the vertex before j on the hull of points
// 1..j) walking up, !FWD the least concave majorant links mj[k] walking down.  AS 217 follows link[link[j]] to pop
// a vertex -- two dependent loads from memory per pop.  The chain j-1, link[j-1], link[link[j-1]], ... is exactly a
// stack, so it is kept as one: (index, value) per vertex, every push written to global memory (stk_i / stk_x, the
// arrays the interval search uses later) and mirrored in a ring of kDipWindow entries per lane in LDS.  A pop reads
// the entry below from LDS (tens of ns) unless the stack fell below the ring, which then refills as it grows.
template <bool FWD>
__device__ __forceinline__ void dip_hull_scan(const float* __restrict__ Xs, int64_t ld, int c, int C, int n,
                                              int32_t* __restrict__ link, int32_t* __restrict__ stk_i,
                                              float* __restrict__ stk_x, int32_t* s_i, float* s_x) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int term = FWD ? 1 : n;   // the vertex no scan pops
    // Offsets move by additions: a wave runs ONE dependent instruction stream per row, so every 64-bit multiply of an
    // index by C or ld is paid in full (the scans are bound by instructions per row).
    const int64_t row_step = FWD ? ld : -ld;        // between consecutive rows of Xs in scan order
    const int64_t link_step = FWD ? (int64_t)C : -(int64_t)C;
    auto slot = [&](int p) -> int { return (int)(((unsigned)p & (unsigned)(kDipWindow - 1)) * kWave) + lane; };
    int top = 1, valid_lo = 1;      // stack positions 1..top; positions >= valid_lo are current in the LDS ring
    int64_t top_off = (int64_t)C + c;   // offset of position `top` in stk_i / stk_x
    auto put = [&](int p, int idx, float v) {    // p == top, top_off its offset
        s_i[slot(p)] = idx;
        s_x[slot(p)] = v;
        stk_i[top_off] = idx;
        stk_x[top_off] = v;
        if (p < valid_lo) valid_lo = p;
        else if (p - kDipWindow + 1 > valid_lo) valid_lo = p - kDipWindow + 1;
    };
    int ia = term, ib = term;       // top of the stack and the vertex below it
    const float xterm = Xs[(int64_t)(term - 1) * ld + c];
    double xa = (double)xterm, xb = xa;
    put(1, term, xterm);
    link[(int64_t)term * C + c] = term;
    // rows are requested a batch ahead of the one in work: clamped, unconditional loads
    int64_t x_off = (int64_t)((FWD ? 2 : n - 1) - 1) * ld + c;   // row of scan position 2
    auto load_batch = [&](float (&dst)[kDipBatch], int t0) {     // t0 <= n; x_off is the offset of scan position t0
#pragma unroll
        for (int u = 0; u < kDipBatch; ++u) {
            dst[u] = Xs[x_off];
            if (t0 + u < n) x_off += row_step;   // stays on the last row once it is reached
        }
    };
    float xnext[kDipBatch];
    load_batch(xnext, 2);
    int64_t link_off = (int64_t)(FWD ? 2 : n - 1) * C + c;
    for (int t0 = 2; t0 <= n; t0 += kDipBatch) {
        float xv[kDipBatch];
#pragma unroll
        for (int u = 0; u < kDipBatch; ++u) xv[u] = xnext[u];
        // after a batch x_off stands at scan position min(t0 + kDipBatch, n)
        load_batch(xnext, t0 + kDipBatch <= n ? t0 + kDipBatch : n);
#pragma unroll
        for (int u = 0; u < kDipBatch; ++u) {
            const int t = t0 + u;
            if (t <= n) {
                const int j = FWD ? t : n + 1 - t;
                const double xj = (double)xv[u];
                while (!(ia == term || (xj - xa) * (double)(ia - ib) < (xa - xb) * (double)(j - ia))) {
                    --top;
                    top_off -= C;
                    ia = ib;
                    xa = xb;
                    if (top >= 2) {
                        // the ring slot is read unconditionally and overridden from memory when it is stale: hipcc turns
                        // "LDS or global" into ONE load through a selected pointer otherwise -- a flat load (seen in the ISA)
                        const int p = top - 1;
                        int ring_i = s_i[slot(p)];
                        float ring_x = s_x[slot(p)];
                        if (p < valid_lo) {   // volatile: keeps this rare path a branch of its own
                            ring_i = *reinterpret_cast<const volatile int32_t*>(stk_i + (top_off - C));
                            ring_x = *reinterpret_cast<const volatile float*>(stk_x + (top_off - C));
                        }
                        ib = ring_i;
                        xb = (double)ring_x;
                    }
                }
                link[link_off] = ia;
                link_off += link_step;
                ++top;
                top_off += C;
                put(top, j, xv[u]);
                ib = ia;
                xb = xa;
                ia = j;
                xa = xj;
            }
        }
    }
}

__global__ __launch_bounds__(kWave) void dip_sorted_kernel(const float* __restrict__ Xs, int64_t n64, int C, int64_t ld,
                                                           int32_t* __restrict__ mn, int32_t* __restrict__ mj,
                                                           int32_t* __restrict__ gcm, int32_t* __restrict__ lcm,
                                                           double* __restrict__ dip_out, int32_t* __restrict__ lo_out,
                                                           int32_t* __restrict__ hi_out, int lanes) {
#pragma clang fp contract(off)
    __shared__ int32_t s_i[kDipWindow * kWave];
    __shared__ float s_x[kDipWindow * kWave];
    // `lanes` columns per wave: the work of a wave is a chain of dependent steps whose length is the longest of its
    // columns', so a matrix of few columns is spread over more, emptier waves (dcv_dip_sorted picks the number)
    const int c = blockIdx.x * lanes + threadIdx.x;
    if ((int)threadIdx.x >= lanes || c >= C) return;
    const int n = (int)n64;
    auto xf = [&](int j) -> float { return Xs[(int64_t)(j - 1) * ld + c]; };
    auto x = [&](int j) -> double { return (double)xf(j); };
    auto at = [&](int j) -> int64_t { return (int64_t)j * C + c; };
    if (n < 2 || !(x(n) != x(1))) {
        dip_out[c] = 0.0;
        lo_out[c] = 0;
        hi_out[c] = n > 0 ? n - 1 : 0;
        return;
    }
    // the two hull scans; gcm / lcm serve as the vertex stack until the interval search below needs them
    dip_hull_scan<true>(Xs, ld, c, C, n, mn, gcm, reinterpret_cast<float*>(lcm), s_i, s_x);
    dip_hull_scan<false>(Xs, ld, c, C, n, mj, gcm, reinterpret_cast<float*>(lcm), s_i, s_x);
    int low = 1, high = n;
    double dipv = 1.0;
    // every pass either ends the search or shrinks [low, high]: at most n passes
    for (int pass = 0; pass <= n; ++pass) {
        gcm[at(1)] = high;
        int i = 1;
        for (int g = high; g > low;) {
            g = mn[at(g)];
            gcm[at(++i)] = g;
        }
        const int l_gcm = i;
        int ig = i, ix = i - 1;
        lcm[at(1)] = low;
        i = 1;
        for (int l = low; l < high;) {
            l = mj[at(l)];
            lcm[at(++i)] = l;
        }
        const int l_lcm = i;
        int ih = i, iv = 2;
        double d = 0.0;
        if (l_gcm != 2 || l_lcm != 2) {
            for (;;) {
                const int gcmix = gcm[at(ix)], lcmiv = lcm[at(iv)];
                if (gcmix > lcmiv) {
                    const int gcmi1 = gcm[at(ix + 1)];
                    const double xg1 = x(gcmi1);
                    const double dx = (double)(lcmiv - gcmi1 + 1) - (x(lcmiv) - xg1) * (double)(gcmix - gcmi1) / (x(gcmix) - xg1);
                    ++iv;
                    if (dx >= d) { d = dx; ig = ix + 1; ih = iv - 1; }
                } else {
                    const int lcmiv1 = lcm[at(iv - 1)];
                    const double xl1 = x(lcmiv1);
                    const double dx = (x(gcmix) - xl1) * (double)(lcmiv - lcmiv1) / (x(lcmiv) - xl1) - (double)(gcmix - lcmiv1 - 1);
                    --ix;
                    if (dx >= d) { d = dx; ig = ix + 1; ih = iv; }
                }
                if (ix < 1) ix = 1;
                if (iv > l_lcm) iv = l_lcm;
                if (gcm[at(ix)] == lcm[at(iv)]) break;
            }
        } else {
            d = 1.0;
        }
        if (d < dipv) break;
        double dip_l = 0.0;
        for (int j = ig; j < l_gcm; ++j) {
            double max_t = 1.0;
            const int jb = gcm[at(j + 1)], je = gcm[at(j)];
            const double xb = x(jb), xe = x(je);
            if (je - jb > 1 && xe != xb) {
                const double Cc = (double)(je - jb) / (xe - xb);
                for (int j0 = jb; j0 <= je; j0 += kDipDeep) {   // kDipDeep loads in flight; a repeated je changes no maximum
                    float xv[kDipDeep];
#pragma unroll
                    for (int u = 0; u < kDipDeep; ++u) xv[u] = xf(j0 + u <= je ? j0 + u : je);
#pragma unroll
                    for (int u = 0; u < kDipDeep; ++u) {
                        const int jj = j0 + u <= je ? j0 + u : je;
                        const double tt = (double)(jj - jb + 1) - ((double)xv[u] - xb) * Cc;
                        if (max_t < tt) max_t = tt;
                    }
                }
            }
            if (dip_l < max_t) dip_l = max_t;
        }
        double dip_u = 0.0;
        for (int j = ih; j < l_lcm; ++j) {
            double max_t = 1.0;
            const int jb = lcm[at(j)], je = lcm[at(j + 1)];
            const double xb = x(jb), xe = x(je);
            if (je - jb > 1 && xe != xb) {
                const double Cc = (double)(je - jb) / (xe - xb);
                for (int j0 = jb; j0 <= je; j0 += kDipDeep) {
                    float xv[kDipDeep];
#pragma unroll
                    for (int u = 0; u < kDipDeep; ++u) xv[u] = xf(j0 + u <= je ? j0 + u : je);
#pragma unroll
                    for (int u = 0; u < kDipDeep; ++u) {
                        const int jj = j0 + u <= je ? j0 + u : je;
                        const double tt = ((double)xv[u] - xb) * Cc - (double)(jj - jb - 1);
                        if (max_t < tt) max_t = tt;
                    }
                }
            }
            if (dip_u < max_t) dip_u = max_t;
        }
        const double dipnew = dip_u > dip_l ? dip_u : dip_l;
        if (dipv < dipnew) dipv = dipnew;
        const int nlow = gcm[at(ig)], nhigh = lcm[at(ih)];
        if (low == nlow && high == nhigh) break;
        low = nlow;
        high = nhigh;
    }
    dip_out[c] = dipv / (double)(2 * (int64_t)n);
    lo_out[c] = low - 1;
    hi_out[c] = high - 1;
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_col_histogram_workspace(int64_t n, int32_t F, int32_t bins) {
    (void)n; (void)F; (void)bins;
    return 0;   // the workgroups add straight into the result
}

extern "C" int dcv_col_histogram(const float* X_d, int64_t n, int32_t F, int64_t ld, const float* edges_d, int32_t bins,
                                 int64_t* counts_d, void* ws_d, size_t ws_bytes, void* stream) {
    (void)ws_d; (void)ws_bytes;
    DCV_REQUIRE(X_d && edges_d && counts_d && n > 0 && F > 0 && ld >= F, "dcv_col_histogram: bad arguments (n=%lld F=%d ld=%lld)",
                (long long)n, F, (long long)ld);
    DCV_REQUIRE(bins >= 1 && bins <= kHistMaxBins, "dcv_col_histogram: bins = %d, supported 1..%d", bins, kHistMaxBins);
    hipStream_t s = as_stream(stream);
    DCV_CHECK_HIP(hipMemsetAsync(counts_d, 0, (size_t)F * bins * sizeof(int64_t), s));
    const int ncb = (int)cdiv(F, kHistCols);
    // rows per workgroup: enough to amortise zeroing and flushing 64 x bins counters, few enough to fill the chip
    int64_t nb = cdiv(n, 2048);
    const int64_t cap = cdiv((int64_t)num_cus() * 12, ncb);
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    const int64_t rpb = cdiv(n, nb);
    nb = cdiv(n, rpb);
    const size_t lds = (size_t)kHistCols * hist_stride(bins) * (sizeof(unsigned int) + sizeof(float));
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts_d);
    if (quad_path(X_d, F, ld))
        hipLaunchKernelGGL(col_histogram_kernel<4>, dim3((unsigned)nb, ncb), dim3(kHistThreads), lds, s, X_d, n, F, ld, edges_d, bins, cnt, rpb);
    else
        hipLaunchKernelGGL(col_histogram_kernel<1>, dim3((unsigned)nb, ncb), dim3(kHistThreads), lds, s, X_d, n, F, ld, edges_d, bins, cnt, rpb);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

extern "C" size_t dcv_dip_sorted_workspace(int64_t n, int32_t C) {
    if (n <= 0 || C <= 0) return 0;
    return (size_t)4 * (size_t)(n + 1) * (size_t)C * sizeof(int32_t);
}

extern "C" int dcv_dip_sorted(const float* Xs_d, int64_t n, int32_t C, int64_t ld, double* dip_d, int32_t* lo_d, int32_t* hi_d,
                              void* ws_d, size_t ws_bytes, void* stream) {
    DCV_REQUIRE(Xs_d && dip_d && lo_d && hi_d && n > 0 && C > 0 && ld >= C, "dcv_dip_sorted: bad arguments (n=%lld C=%d ld=%lld)",
                (long long)n, C, (long long)ld);
    DCV_REQUIRE(n < ((int64_t)1 << 31) - 1, "dcv_dip_sorted: n = %lld does not fit 31 bits", (long long)n);
    DCV_REQUIRE(ws_d && ws_bytes >= dcv_dip_sorted_workspace(n, C), "dcv_dip_sorted: workspace too small");
    int32_t* w = static_cast<int32_t*>(ws_d);
    const size_t per = (size_t)(n + 1) * (size_t)C;
    // columns per wave: 64 when the columns alone give every SIMD a wave, fewer (down to 8) otherwise -- the kernel is bound by
    // the latency of each wave's dependent chain, not by lanes
    int lanes = kWave;
    while (lanes > 8 && cdiv(C, lanes / 2) <= (int64_t)num_cus() * 4) lanes /= 2;
    hipLaunchKernelGGL(dip_sorted_kernel, dim3((unsigned)cdiv(C, lanes)), dim3(kWave), 0, as_stream(stream), Xs_d, n, C, ld, w, w + per,
                       w + 2 * per, w + 3 * per, dip_d, lo_d, hi_d, lanes);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

// Shared pieces of the float64 point kernels (kmeans.hip, scores.hip, linkage.hip, hdbscan.hip), ONE copy each: the
// plumbing of a streaming pass, the exact squared distance, the (value, index) argmin within a wave, a workgroup and the
// grid, and on the host the workspace layout, its size refusal and the loop over blocks of one-launch steps.
#pragma once
#include "common.h"
#include "handoff.h"

namespace dcv {

constexpr int kPtThreads = 256;     // workgroup size of everything below
constexpr int kPtMaxD = 16;         // coordinates per point
constexpr int kPtMaxBlocks = 1024;  // workgroups of a streaming pass (sizes the partials' workspace)

// ------------------------------------------------------------------ streaming passes
// workgroups of a streaming pass over n points: 1024 points each, four per CU at most
inline int point_blocks(int64_t n) {
    int64_t b = cdiv(n, (int64_t)kPtThreads * 4);
    const int64_t cap = (int64_t)num_cus() * 4;
    if (b > cap) b = cap;
    if (b > kPtMaxBlocks) b = kPtMaxBlocks;
    if (b < 1) b = 1;
    return (int)b;
}

// acc[i] = sum over the blocks of part[b][i], i < width (defined in kmeans.hip): one workgroup per output, its threads take
// b = t, t + 256, ... (all loads in flight at once; one thread walking 1024 partials with dependent loads cost 0.4 ms -- most
// of a k-means pass) and block_sum adds them up.  The caller checks the launch.
void sum_blocks(const double* part, int nblocks, int width, double* acc, hipStream_t s);

__device__ __forceinline__ void load_point(const double* __restrict__ P, int64_t i, int d, double* x) {
    const double* p = P + i * d;
    if ((d & 1) == 0) {
#pragma unroll
        for (int c = 0; c < kPtMaxD; c += 2) {
            if (c < d) {
                const double2 v = *reinterpret_cast<const double2*>(p + c);
                x[c] = v.x;
                x[c + 1] = v.y;
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < kPtMaxD; ++c)
            if (c < d) x[c] = p[c];
    }
}
template <int D>
__device__ __forceinline__ void load_point(const double* __restrict__ P, int64_t i, double (&x)[D]) {
    const double* p = P + i * D;
    if constexpr (D % 2 == 0) {
#pragma unroll
        for (int c = 0; c < D; c += 2) {
            const double2 v = *reinterpret_cast<const double2*>(p + c);
            x[c] = v.x;
            x[c + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = p[c];
    }
}

// s_red[0] = the sum of the block's 256 values v by a fixed LDS tree (pairs 128 apart, then 64, ...), valid after the call
__device__ __forceinline__ void block_sum(double v, double (&s_red)[kPtThreads], int t) {
    s_red[t] = v;
    __syncthreads();
    for (int o = kPtThreads / 2; o > 0; o >>= 1) {
        if (t < o) s_red[t] += s_red[t + o];
        __syncthreads();
    }
}

// ------------------------------------------------------------------ exact squared distance
// sum_q (a[q] - p[q])^2 over q < d, the squares added in coordinate order, every product and every sum rounded on its own
// (no fma): what scipy's pdist and scikit-learn's distance metrics compute.  `a` sits in registers, `p` is read through the
// pointer (LDS or global memory), every coordinate once.  Plain operators under the pragma: the __dmul_rn / __dadd_rn
// wrappers are inlined with the default contraction and fuse into one fma (seen in the ISA), so never use them here.
// The primitive takes TWO register operands against the one pointer (the distance matrix fills two columns per loaded row
// value); P_FIRST: the differences are p[q] - a[q].
template <int MAXD, bool P_FIRST>
__device__ __forceinline__ void sqdist_exact2(const double (&a)[MAXD], const double (&b)[MAXD], const double* p, int d, double& sa, double& sb) {
#pragma clang fp contract(off)
    sa = 0.0;
    sb = 0.0;
#pragma unroll
    for (int q = 0; q < MAXD; ++q)
        if (q < d) {
            const double x = p[q];
            const double da = P_FIRST ? x - a[q] : a[q] - x, db = P_FIRST ? x - b[q] : b[q] - x;
            const double qa = da * da, qb = db * db;
            sa = sa + qa;
            sb = sb + qb;
        }
}
template <int MAXD>
__device__ __forceinline__ double sqdist_exact(const double (&a)[MAXD], const double* p, int d) {
    double s, same;
    sqdist_exact2<MAXD, false>(a, a, p, d, s, same);   // the second sum is the first: nothing is computed twice
    return s;
}

// ------------------------------------------------------------------ argmin
// A candidate of the per-step kernels: (value, index) and, with PAYLOAD, one int that rides along (never compared).
// An index < 0 is "no candidate": it loses against everything, whatever its value.
template <bool PAYLOAD>
struct Cand {
    double v;
    int i, p;
};
template <>
struct Cand<false> {   // no payload: nothing to carry through the shuffles
    double v;
    int i;
};
// LDS of the block reduction and the ticket
template <bool PAYLOAD>
struct ArgminLds {
    double v[kPtThreads / kWave];
    int i[kPtThreads / kWave];
    int p[PAYLOAD ? kPtThreads / kWave : 1];
    unsigned flag;
    __device__ __forceinline__ Cand<PAYLOAD> get(int w) const {
        if constexpr (PAYLOAD) return {v[w], i[w], p[w]};
        else return {v[w], i[w]};
    }
};

// lexicographic minimum of (value, index)
template <bool PAYLOAD>
__device__ __forceinline__ void argmin_take(Cand<PAYLOAD>& b, const Cand<PAYLOAD>& o) {
    if (o.i >= 0 && (b.i < 0 || o.v < b.v || (o.v == b.v && o.i < b.i))) b = o;
}

// every thread of the 256 ends up with the workgroup's minimum: shuffles within a wave, then the waves through LDS
template <bool PAYLOAD>
__device__ __forceinline__ void block_argmin(Cand<PAYLOAD>& b, ArgminLds<PAYLOAD>& s) {
    for (int off = kWave / 2; off > 0; off >>= 1) {
        Cand<PAYLOAD> o;
        o.v = __shfl_down(b.v, off);
        o.i = __shfl_down(b.i, off);
        if constexpr (PAYLOAD) o.p = __shfl_down(b.p, off);
        argmin_take(b, o);
    }
    const int w = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
        s.v[w] = b.v;
        s.i[w] = b.i;
        if constexpr (PAYLOAD) s.p[w] = b.p;
    }
    __syncthreads();
    b = s.get(0);
    for (int k = 1; k < kPtThreads / kWave; ++k) argmin_take(b, s.get(k));
    __syncthreads();
}

// Grid-wide argmin inside one launch (at most kPtThreads workgroups of kPtThreads threads; every thread calls it with its
// own candidate).  Each workgroup reduces, hands its candidate over in `part` (2 doubles per workgroup, 3 with PAYLOAD; the
// ints travel as exact doubles) and takes a ticket; the last to arrive loads one partial per thread and reduces again.
// Returns true in every thread of that last workgroup, with the grid's minimum in `c`.  The order around the ticket is the
// one handoff.h documents: sc1 stores, s_waitcnt vmcnt(0), barrier, ticket, acquire, wait, barrier, sc1 loads.
template <bool PAYLOAD>
__device__ __forceinline__ bool ticketed_argmin(Cand<PAYLOAD>& c, double* part, unsigned* ticket, ArgminLds<PAYLOAD>& s) {
    constexpr int W = PAYLOAD ? 3 : 2;
    block_argmin(c, s);
    if (threadIdx.x == 0) {
        handoff_store(part + W * blockIdx.x, c.v);
        handoff_store(part + W * blockIdx.x + 1, (double)c.i);
        if constexpr (PAYLOAD) handoff_store(part + W * blockIdx.x + 2, (double)c.p);
    }
    if (!handoff_arrive_last(ticket, gridDim.x, &s.flag)) return false;
    c.i = -1;
    if (threadIdx.x < gridDim.x) {
        c.v = handoff_load(part + W * threadIdx.x);
        c.i = (int)handoff_load(part + W * threadIdx.x + 1);
        if constexpr (PAYLOAD) c.p = (int)handoff_load(part + W * threadIdx.x + 2);
    }
    block_argmin(c, s);
    return true;
}

// The k-means passes' form of the same minimum, kept apart on purpose: rows are int64 (n is not bounded by 2^31 there),
// the empty index is INT64_MAX (it loses every tie, so there is no "index < 0" rule), and only lane 0 ends up with the
// wave's minimum.  An int64 index costs two shuffles per round: the per-step kernels above do not pay for it.
__device__ __forceinline__ void take_min(double& best, int64_t& besti, double v, int64_t i) {
    if (v < best || (v == best && i < besti)) {
        best = v;
        besti = i;
    }
}
__device__ __forceinline__ void wave_min(double& best, int64_t& besti) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_down(best, off, 64);
        const int64_t i2 = __shfl_down(besti, off, 64);
        take_min(best, besti, v2, i2);
    }
}

// ------------------------------------------------------------------ host: workspace layout
// Carves a workspace into regions that each start on a 256-byte boundary; `total` is the end of the last one.
template <class T>
struct Region {
    size_t off;
    T* in(void* ws) const { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }
};
struct Carver {
    size_t total = 0;
    template <class T>
    Region<T> take(size_t count) {
        const size_t off = align_up(total, 256);
        total = off + count * sizeof(T);
        return {off};
    }
};

// slice and grid of a per-step kernel over `len` items: one workgroup per CU at most, each a whole number of `quantum`
// items; never more than kPtThreads workgroups (the last arriver of ticketed_argmin reads one partial per thread)
struct StepGrid {
    int per, grid;
};
inline StepGrid step_grid(int64_t len, int quantum, int cus) {
    const int cap = cus < kPtThreads ? (cus > 0 ? cus : 1) : kPtThreads;
    StepGrid g;
    g.per = (int)align_up((size_t)cdiv(len, cap), (size_t)quantum);
    g.grid = (int)cdiv(len, g.per);
    return g;
}

// refuses a missing or short workspace: "<entry>: workspace of X bytes, Y needed", DCV_ENOMEM (the text of the clustering
// entries; common.h's DCV_REQUIRE_WORKSPACE says "workspace too small (X bytes, need Y)")
#define DCV_REQUIRE_POINTS_WORKSPACE(entry, ws, bytes, needed)                                                     \
    do {                                                                                                           \
        const size_t _need = (needed);                                                                             \
        if (!(ws) || (bytes) < _need) {                                                                            \
            dcv::set_error(entry ": workspace of %zu bytes, %zu needed", (size_t)(bytes), _need);                  \
            return DCV_ENOMEM;                                                                                     \
        }                                                                                                          \
    } while (0)

// Runs a chain of one-launch steps whose device state starts with the words of Head (which has `done` and `error`):
// enqueues block(h, left) steps with launch() (left = cap - steps enqueued so far), copies the head of the state back into
// h, synchronises, and repeats until done, error or cap.  Nothing waits on the device inside a block: steps enqueued past
// the end, or after an error, return at once.
template <class Head, class Block, class Launch>
int run_steps(hipStream_t s, const void* state_d, Head& h, int64_t cap, Block&& block, Launch&& launch) {
    int64_t enqueued = 0;
    while (!h.done && !h.error && enqueued < cap) {
        const int64_t steps = block(h, cap - enqueued);
        for (int64_t k = 0; k < steps; ++k) launch();
        DCV_CHECK_LAUNCH();
        enqueued += steps;
        DCV_CHECK_HIP(hipMemcpyAsync(&h, state_d, sizeof(h), hipMemcpyDeviceToHost, s));
        DCV_CHECK_HIP(hipStreamSynchronize(s));
    }
    return DCV_OK;
}

}  // namespace dcv

// HDBSCAN (Euclidean, alpha = 1): the two stages of sklearn.cluster.HDBSCAN's kd_tree branch (_hdbscan_prims) that touch
// the points, reproduced bit for bit, so that the minimum spanning tree -- sources, targets and weights, in Prim order --
// is the one scikit-learn hands to its (host-side) tree condensation.
//
//   core     core[i] = the k-th smallest of sqrt(sum_c (P[i][c] - P[j][c])^2) over ALL j (i itself included): one lane per
//            query, the points streamed through LDS in tiles, a sorted list of the k smallest SQUARED sums per lane in LDS
//            (entry e of lane t at [e * 64 + t]: no bank conflicts; the LDS of a launch is sized by k and d), one correctly
//            rounded sqrt of the k-th at the end.
//            The squares are added in coordinate order, every product and sum rounded on its own (no fma):
//            sqdist_exact (points.h), as in linkage.hip's distance matrix.
//   step     one launch per step of Prim's algorithm over the implicit mutual-reachability graph
//            mrd(c, j) = max(core[c], core[j], dist(c, j)).  Every workgroup owns a contiguous slice of the points and is
//            the only one to read or write that slice's running minimum, source and in-tree flag (the owner of the current
//            node c marks it).  It lowers the minima against c with a strict '<', reduces its slice to the lexicographic
//            minimum of (value, index), and hands (value, index, source) over (ticketed_argmin, points.h).  The last workgroup
//            to arrive combines the partials, appends the edge and names the next current node in the state.
//
// Nothing waits on another workgroup: the host enqueues exactly n - 1 steps in blocks and reads a few words of state
// between blocks; steps enqueued after an error return at once.  The state is O(n): no n x n matrix.
#include <cfloat>
#include <vector>

#include "points.h"

namespace dcv {

constexpr int kHdMaxD = kPtMaxD;
constexpr int kHdMaxK = 64;                  // min_samples the core-distance kernel holds per lane
constexpr int kCoreLanes = 64;               // queries per workgroup: one wave
constexpr int kCoreTile = 128;               // points per LDS tile
constexpr int kMstThreads = kPtThreads;
constexpr int64_t kHdMaxN = ((int64_t)1 << 31) - 1;   // indices travel as int32 and as exact doubles
constexpr size_t kCoreWsBytes = 256;         // one status word

__global__ __launch_bounds__(kCoreLanes) void core_distances_kernel(const double* __restrict__ P, int64_t n, int d, int k,
                                                                     double* __restrict__ core, int32_t* __restrict__ status) {
    extern __shared__ double s_core[];          // k * 64 list entries, then a tile of 128 * d coordinates: 48 KB at most
    double* s_list = s_core;
    double* s_pts = s_core + k * kCoreLanes;
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kCoreLanes + t;
    const bool live = i < n;
    const int64_t iq = live ? i : n - 1;   // a lane past the end works on the last point and stores nothing
    double q[kHdMaxD];
#pragma unroll
    for (int c = 0; c < kHdMaxD; ++c) q[c] = c < d ? P[iq * d + c] : 0.0;
    for (int e = 0; e < k; ++e) s_list[e * kCoreLanes + t] = INFINITY;
    double worst = INFINITY;   // s_list[k - 1] of this lane
    for (int64_t base = 0; base < n; base += kCoreTile) {
        const int cnt = n - base < kCoreTile ? (int)(n - base) : kCoreTile;
        __syncthreads();
        for (int x = t; x < cnt * d; x += kCoreLanes) s_pts[x] = P[base * d + x];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double s = sqdist_exact(q, s_pts + j * d, d);   // the same address in every lane: an LDS broadcast
            if (s < worst) {   // a NaN never enters
                int e = k - 1;
                for (; e > 0; --e) {
                    const double up = s_list[(e - 1) * kCoreLanes + t];
                    if (!(up > s)) break;
                    s_list[e * kCoreLanes + t] = up;
                }
                s_list[e * kCoreLanes + t] = s;
                worst = s_list[(k - 1) * kCoreLanes + t];
            }
        }
    }
    if (live) {
        // k <= n finite squared sums fill the list; what is left at infinity came from non-finite points
        if (!(worst < INFINITY)) *status = 1;
        core[i] = __dsqrt_rn(worst);
    }
}

// Prim state in device memory.  The first four words are what the host reads between blocks of steps.
struct MstState {
    int32_t edges;     // edges recorded so far
    int32_t done;      // n - 1 edges recorded: every later step is a no-op
    int32_t error;     // 1 = a step found no candidate
    int32_t current;   // the node the next step scans from (in the tree; its owner marks it)
    unsigned ticket;
    unsigned pad[3];
};

__global__ void mst_init_kernel(MstState* __restrict__ st, double* __restrict__ min_reach, int32_t* __restrict__ source,
                                int32_t* __restrict__ in_tree, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        min_reach[i] = INFINITY;
        source[i] = 1;   // as scikit-learn starts; never read before a finite minimum has replaced it
        in_tree[i] = 0;
    }
    if (i == 0) {
        MstState s = {};
        *st = s;
    }
}

// One step of Prim's algorithm from the current node c, as sklearn's mst_from_data_matrix runs it: for every j outside
// the tree, m = max(core[c], core[j], dist(c, j)); a strictly smaller m replaces min_reach[j] (source c); the candidate
// of j is its (updated) minimum, and the new node is the lowest index among the candidates of minimal value --
// scikit-learn scans upwards with a strict '<' from DBL_MAX, so an infinite minimum is never a candidate.
__global__ __launch_bounds__(kMstThreads) void mst_step_kernel(MstState* __restrict__ st, const double* __restrict__ P,
                                                               const double* __restrict__ core, double* __restrict__ min_reach,
                                                               int32_t* __restrict__ source, int32_t* __restrict__ in_tree,
                                                               int32_t* __restrict__ e_src, int32_t* __restrict__ e_dst,
                                                               double* __restrict__ e_w, double* __restrict__ part, int n, int d,
                                                               int per) {
    __shared__ ArgminLds<true> s_min;
    if (st->done | st->error) return;   // uniform over the grid: the state only changes behind every workgroup's ticket
    // what the last arriver needs, read ahead of the ticket by everybody
    const int nedge = st->edges;
    const int c = st->current;
    const double cc = core[c];
    double pc[kHdMaxD];
#pragma unroll
    for (int q = 0; q < kHdMaxD; ++q) pc[q] = q < d ? P[(int64_t)c * d + q] : 0.0;

    const int begin = blockIdx.x * per;
    const int end = n - begin < per ? n : begin + per;   // begin < n: the grid is cdiv(n, per)
    Cand<true> best = {DBL_MAX, -1, -1};   // (minimum, node, its source)
    for (int64_t j = begin + (int)threadIdx.x; j < end; j += kMstThreads) {   // upwards within a lane; 64-bit: no wrap near 2^31
        if (in_tree[j]) continue;
        if (j == c) {
            in_tree[j] = 1;
            continue;
        }
        const double s = sqdist_exact(pc, P + j * d, d);
        double m = cc;
        const double cj = core[j];
        if (cj > m) m = cj;
        const double dist = __dsqrt_rn(s);
        if (dist > m) m = dist;
        double mr = min_reach[j];
        int sj = source[j];
        if (m < mr) {
            mr = m;
            sj = c;
            min_reach[j] = m;
            source[j] = c;
        }
        if (mr < best.v) best = {mr, (int)j, sj};
    }
    if (!ticketed_argmin(best, part, &st->ticket, s_min) || threadIdx.x != 0) return;
    const double md = best.v;
    const int mi = best.i, ms = best.p;
    if (mi < 0 || nedge >= n - 1) {   // nothing comparable outside the tree: non-finite input; never write past the edges
        st->error = 1;
        return;
    }
    e_src[nedge] = ms;
    e_dst[nedge] = mi;
    e_w[nedge] = md;
    st->edges = nedge + 1;
    st->current = mi;
    if (nedge + 1 == n - 1) st->done = 1;
}

struct MstLayout {   // the regions in workspace order
    MstLayout(int64_t n_, int cus) : n((size_t)n_), g(step_grid(n_, kMstThreads, cus)) {}
    size_t n;
    StepGrid g;   // one workgroup covers a whole number of passes of its threads
    Carver c;
    Region<MstState> state = c.take<MstState>(1);
    Region<double> reach = c.take<double>(n);
    Region<int32_t> source = c.take<int32_t>(n), tree = c.take<int32_t>(n), esrc = c.take<int32_t>(n), edst = c.take<int32_t>(n);
    Region<double> ew = c.take<double>(n), part = c.take<double>(3 * kMstThreads);
};

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_core_distances_workspace(int64_t n, int32_t d, int32_t k) {
    if (n < 2 || n > kHdMaxN || d < 1 || d > kHdMaxD || k < 1 || k > kHdMaxK || k > n) return 0;
    return kCoreWsBytes;
}

extern "C" int dcv_core_distances(const double* P_d, int64_t n, int32_t d, int32_t k, double* core_d, void* ws_d, size_t ws_bytes,
                                  void* stream) {
    DCV_REQUIRE(n >= 2 && n <= kHdMaxN, "dcv_core_distances: n = %lld, supported 2..%lld", (long long)n, (long long)kHdMaxN);
    DCV_REQUIRE(d >= 1 && d <= kHdMaxD, "dcv_core_distances: d = %d, supported 1..%d", d, kHdMaxD);
    DCV_REQUIRE(k >= 1 && k <= kHdMaxK && k <= n, "dcv_core_distances: k = %d, supported 1..min(n, %d)", k, kHdMaxK);
    DCV_REQUIRE(P_d && core_d, "dcv_core_distances: null points or result");
    DCV_REQUIRE_POINTS_WORKSPACE("dcv_core_distances", ws_d, ws_bytes, kCoreWsBytes);
    hipStream_t s = as_stream(stream);
    int32_t* status = static_cast<int32_t*>(ws_d);
    DCV_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    const size_t lds = ((size_t)k * kCoreLanes + (size_t)kCoreTile * d) * sizeof(double);   // sized by k and d: small k, many waves per CU
    hipLaunchKernelGGL(core_distances_kernel, dim3((unsigned)cdiv(n, kCoreLanes)), dim3(kCoreLanes), lds, s, P_d, n, (int)d, (int)k, core_d,
                       status);
    DCV_CHECK_LAUNCH();
    int32_t h = 0;
    DCV_CHECK_HIP(hipMemcpyAsync(&h, status, sizeof(h), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    DCV_REQUIRE(h == 0, "dcv_core_distances: a point has fewer than %d finite distances: non-finite input?", k);
    return DCV_OK;
}

extern "C" size_t dcv_mr_mst_workspace(int64_t n, int32_t d) {
    if (n < 2 || n > kHdMaxN || d < 1 || d > kHdMaxD) return 0;
    // no offset depends on the CU count (only `per` does): one size for every device
    return MstLayout(n, kMstThreads).c.total;
}

extern "C" int dcv_mr_mst(const double* P_d, int64_t n, int32_t d, const double* core_d, int64_t* src_h, int64_t* dst_h, double* w_h,
                          void* ws_d, size_t ws_bytes, void* stream) {
    DCV_REQUIRE(n >= 2 && n <= kHdMaxN, "dcv_mr_mst: n = %lld, supported 2..%lld", (long long)n, (long long)kHdMaxN);
    DCV_REQUIRE(d >= 1 && d <= kHdMaxD, "dcv_mr_mst: d = %d, supported 1..%d", d, kHdMaxD);
    DCV_REQUIRE(P_d && core_d && src_h && dst_h && w_h, "dcv_mr_mst: null points, core distances or result");
    DCV_REQUIRE_POINTS_WORKSPACE("dcv_mr_mst", ws_d, ws_bytes, dcv_mr_mst_workspace(n, d));
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(ws_d) & 7) == 0, "dcv_mr_mst: workspace not 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const MstLayout L(n, num_cus());
    MstState* st = L.state.in(ws_d);
    double* min_reach = L.reach.in(ws_d);
    int32_t* source = L.source.in(ws_d);
    int32_t* in_tree = L.tree.in(ws_d);
    int32_t* e_src = L.esrc.in(ws_d);
    int32_t* e_dst = L.edst.in(ws_d);
    double* e_w = L.ew.in(ws_d);

    hipLaunchKernelGGL(mst_init_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, st, min_reach, source, in_tree, n);
    DCV_CHECK_LAUNCH();

    struct {
        int32_t edges, done, error, current;
    } h = {0, 0, 0, 0};
    const int64_t total = n - 1;   // every step records exactly one edge or sets the error word
    const int rc = run_steps(
        s, st, h, total, [](const auto&, int64_t left) { return left < 4096 ? left : (int64_t)4096; },
        [&] {
            hipLaunchKernelGGL(mst_step_kernel, dim3(L.g.grid), dim3(kMstThreads), 0, s, st, P_d, core_d, min_reach, source, in_tree, e_src, e_dst,
                               e_w, L.part.in(ws_d), (int)n, (int)d, L.g.per);
        });
    if (rc) return rc;
    DCV_REQUIRE(h.error == 0 && h.done, "dcv_mr_mst: the tree did not finish (%s; %d of %lld edges): non-finite input?",
                h.error ? "a step found no candidate" : "steps missing", h.edges, (long long)total);

    std::vector<int32_t> a((size_t)total), b((size_t)total);
    DCV_CHECK_HIP(hipMemcpyAsync(a.data(), e_src, a.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipMemcpyAsync(b.data(), e_dst, b.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipMemcpyAsync(w_h, e_w, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < total; ++i) {
        src_h[i] = a[(size_t)i];
        dst_h[i] = b[(size_t)i];
    }
    return DCV_OK;
}

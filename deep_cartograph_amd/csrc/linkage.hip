// Agglomerative clustering (complete / average / ward, Euclidean): the nearest-neighbour chain of
// scipy.cluster.hierarchy.linkage over a device-resident SQUARE float64 distance matrix, reproduced bit for bit
// (ties included), so that the dendrogram -- and every cut of it -- is the one scikit-learn's
// AgglomerativeClustering returns.
//
//   pdist    D[i][j] = sqrt(sum_c (P[i][c] - P[j][c])^2), the squares added in coordinate order, every product and sum
//            rounded on its own (no fma), correctly rounded sqrt.  Rows are `ld` doubles apart (n rounded up to 16), so
//            every row starts on a 128-byte line and is read with 16-byte loads.
//   step     one launch per chain step.  Head: the row update of the merge the previous step recorded (Lance-Williams
//            on row y and column y).  Body: every workgroup reads the chain state the previous launch left, scans its
//            contiguous slice of row x = top of the chain (dead clusters and x itself masked by `size`), reduces to the
//            lexicographic minimum of (distance, index) and hands it over (ticketed_argmin, points.h).  The last workgroup to
//            arrive combines the partials, applies scipy's rule "the previous chain element wins unless something is strictly
//            closer" and either pushes the neighbour or records the merge, retires x, and describes the row update
//            that is now due in the state.
//
// Nothing waits on another workgroup: the host enqueues a bounded number of steps and reads a few words of state
// between blocks of them; steps enqueued past the end, or after an error, return at once.
#include <algorithm>
#include <numeric>
#include <vector>

#include "points.h"

namespace dcv {

constexpr int kLkThreads = kPtThreads;
constexpr int kLkSlice = 2 * kLkThreads;   // doubles of a row one workgroup covers per pass (16-byte loads)
constexpr int kLkMaxD = kPtMaxD;
constexpr int kLkPdRows = 8;               // rows of the matrix per pdist workgroup

enum { kLkComplete = 0, kLkAverage = 1, kLkWard = 2 };

// Chain state in device memory.  The first six words are what the host reads between blocks of steps.
struct LinkState {
    int32_t merges;      // merges recorded so far
    int32_t done;        // n - 1 merges recorded: every later step is a no-op
    int32_t error;       // 1 = a search found no candidate, 2 = more than 3 (n - 1) searches
    int32_t chain_len;
    int64_t searches;
    int32_t cursor;      // no live index below it (monotone)
    int32_t pending;     // the last step recorded a merge: the head of the next one applies it
    int32_t px, py, pnx, pny;
    double pdxy;
    unsigned ticket;
    unsigned pad;
};

struct dbl2 {
    double a, b;
};

__global__ __launch_bounds__(kLkThreads) void linkage_pdist_kernel(const double* __restrict__ P, int64_t n, int d, int64_t ld,
                                                                    double* __restrict__ D, int col_blocks) {
    const int64_t rb = blockIdx.x / col_blocks;
    const int cb = blockIdx.x - rb * col_blocks;
    const int64_t j = (int64_t)cb * kLkSlice + 2 * threadIdx.x;
    if (j >= n) return;
    const bool two = j + 1 < n;
    double a[kLkMaxD], b[kLkMaxD];
#pragma unroll
    for (int q = 0; q < kLkMaxD; ++q) {
        a[q] = q < d ? P[j * d + q] : 0.0;
        b[q] = (q < d && two) ? P[(j + 1) * d + q] : 0.0;
    }
    const int64_t r0 = rb * kLkPdRows;
    for (int r = 0; r < kLkPdRows; ++r) {
        const int64_t i = r0 + r;
        if (i >= n) break;
        double sa, sb;
        sqdist_exact2<kLkMaxD, true>(a, b, P + i * d, d, sa, sb);   // P[i] - P[j], P[i] - P[j + 1]: row i is loaded once
        dbl2 v;
        v.a = __dsqrt_rn(sa);
        v.b = __dsqrt_rn(sb);
        *reinterpret_cast<dbl2*>(D + i * ld + j) = v;   // j even and j + 1 < ld: inside the row; column n of an odd n is padding
    }
}

__global__ void linkage_init_kernel(LinkState* __restrict__ st, int32_t* __restrict__ size, int32_t* __restrict__ chain, int64_t n,
                                    int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < ld) size[i] = i < n ? 1 : 0;   // the padding of a row is dead from the start
    if (i == 0) {
        LinkState s = {};
        s.chain_len = 1;
        *st = s;
        chain[0] = 0;
    }
}

template <int METHOD>
__device__ __forceinline__ double lk_new_dist(double dxi, double dyi, double dxy, int nx, int ny, int ni) {
#pragma clang fp contract(off)
    if constexpr (METHOD == kLkComplete) {
        return dxi > dyi ? dxi : dyi;
    } else if constexpr (METHOD == kLkAverage) {
        const double a = (double)nx * dxi, b = (double)ny * dyi;
        return (a + b) / (double)(nx + ny);
    } else {
        const double t = 1.0 / (double)(nx + ny + ni);
        const double u = (double)(ni + nx) * t * dxi * dxi;
        const double v = (double)(ni + ny) * t * dyi * dyi;
        const double w = (double)ni * t * dxy * dxy;
        return __dsqrt_rn(u + v - w);
    }
}

// One chain step.  Head: the row update of the merge the PREVIOUS step recorded (ux dead, uy the merged cluster), every
// workgroup on its own slice -- row uy (16-byte stores) and column uy (strided).  Body: the search of row x, the top of
// the chain.  Both in one launch without one workgroup reading what another writes:
//   x == uy   the searched row is the updated one: a workgroup searches the values it has just computed;
//   x != uy   the only updated entry the search touches is D[x][uy].  Nobody stores it while the workgroups run (the
//             owner of row x skips that one column entry); every workgroup derives it from the old D[x][ux] and
//             D[x][uy] (v_fix: the same arithmetic on the same operands as row uy's entry x, the matrix is symmetric
//             bit for bit), the owner of column uy searches with it, and the last arriver stores it behind the ticket.
template <int METHOD>
__global__ __launch_bounds__(kLkThreads) void linkage_step_kernel(LinkState* __restrict__ st, double* __restrict__ D,
                                                                   int32_t* __restrict__ size, int32_t* __restrict__ chain,
                                                                   double* __restrict__ merges, double* __restrict__ part, int n,
                                                                   int64_t ld, int per, int64_t max_searches) {
    __shared__ ArgminLds<false> s_min;
    if (st->done | st->error) return;   // uniform over the grid: the state only changes behind every workgroup's ticket
    const int len = st->chain_len;
    const int x = chain[len - 1];
    const double* row = D + (int64_t)x * ld;
    // what the last arriver needs, read ahead of the ticket by everybody
    const int p = len > 1 ? chain[len - 2] : -1;
    double dp = p >= 0 ? row[p] : 0.0;
    const int sx = size[x];
    const int sp = p >= 0 ? size[p] : 0;
    const int cursor = st->cursor;
    const int nmerge = st->merges;
    const int64_t nsearch = st->searches;
    const bool pend = st->pending != 0;
    const int ux = st->px, uy = st->py, unx = st->pnx, uny = st->pny;
    const double udxy = st->pdxy;
    const bool fix = pend && x != uy;
    double v_fix = 0.0;
    if (fix) {
        v_fix = lk_new_dist<METHOD>(row[ux], row[uy], udxy, unx, uny, sx);
        if (p == uy) dp = v_fix;
    }

    const double* rx = D + (int64_t)(pend ? ux : 0) * ld;
    double* ry = D + (int64_t)(pend ? uy : 0) * ld;
    const int begin = blockIdx.x * per;
    const int end = begin + per < (int)ld ? begin + per : (int)ld;
    Cand<false> best = {INFINITY, -1};   // scipy starts from infinity: a NaN or an infinite distance is never a candidate
    for (int i = begin + 2 * threadIdx.x; i < end; i += kLkSlice) {   // i even, ld even: i + 1 < ld
        dbl2 v = *reinterpret_cast<const dbl2*>(row + i);
        const int2 s = *reinterpret_cast<const int2*>(size + i);
        if (pend) {
            // size[ux] is 0 already; a live i is a row of the matrix (the padding is dead)
            const bool l0 = s.x > 0 && i != uy, l1 = s.y > 0 && i + 1 != uy;
            if (l0 || l1) {
                const dbl2 vx = *reinterpret_cast<const dbl2*>(rx + i);
                dbl2 vy = *reinterpret_cast<const dbl2*>(ry + i);
                if (l0) {
                    vy.a = lk_new_dist<METHOD>(vx.a, vy.a, udxy, unx, uny, s.x);
                    if (i != x) D[(int64_t)i * ld + uy] = vy.a;
                }
                if (l1) {
                    vy.b = lk_new_dist<METHOD>(vx.b, vy.b, udxy, unx, uny, s.y);
                    if (i + 1 != x) D[(int64_t)(i + 1) * ld + uy] = vy.b;
                }
                *reinterpret_cast<dbl2*>(ry + i) = vy;
                if (!fix) v = vy;   // the searched row is row uy itself
            }
            if (fix && i == uy) v.a = v_fix;
            if (fix && i + 1 == uy) v.b = v_fix;
        }
        // upwards with a strict '<', as scipy scans
        if (s.x > 0 && i != x && v.a < best.v) best = {v.a, i};
        if (s.y > 0 && i + 1 != x && v.b < best.v) best = {v.b, i + 1};
    }
    if (!ticketed_argmin(best, part, &st->ticket, s_min) || threadIdx.x != 0) return;
    const double md = best.v;
    const int mi = best.i;
    if (fix) D[(int64_t)x * ld + uy] = v_fix;   // every workgroup has read the old entry: all of them are behind their tickets
    st->searches = nsearch + 1;
    if (mi < 0 && p < 0) {   // nothing comparable in the row: non-finite input
        st->error = 1;
        st->pending = 0;
        return;
    }
    if (p >= 0 && !(mi >= 0 && md < dp)) {
        // the previous element is a nearest neighbour of x as well: merge the pair (smaller index first; it dies)
        const int a = x < p ? x : p, b = x < p ? p : x;
        const int na = x < p ? sx : sp, nb = x < p ? sp : sx;
        double* z = merges + 4 * (int64_t)nmerge;
        z[0] = (double)a;
        z[1] = (double)b;
        z[2] = dp;
        z[3] = (double)(na + nb);
        size[a] = 0;
        size[b] = na + nb;
        st->px = a;
        st->py = b;
        st->pnx = na;
        st->pny = nb;
        st->pdxy = dp;
        st->pending = 1;
        st->merges = nmerge + 1;
        int nlen = len - 2;
        if (nmerge + 1 == n - 1) {
            st->done = 1;
        } else if (nlen == 0) {
            int c = cursor;
            while (c < n && (c == a || size[c] == 0)) ++c;   // monotone: n steps over the whole run
            if (c >= n) {   // cannot happen while merges are missing; never index a row that is not there
                st->error = 2;
                return;
            }
            st->cursor = c;
            chain[0] = c;
            nlen = 1;
        }
        st->chain_len = nlen;
    } else {
        st->pending = 0;
        if (len >= n) {   // a chain never holds a cluster twice, so this is unreachable; never write past the chain
            st->error = 2;
            return;
        }
        chain[len] = mi;
        st->chain_len = len + 1;
    }
    if (nsearch + 1 >= max_searches && !st->done) st->error = 2;   // the chain needs at most 3 (n - 1) searches
}

struct LinkLayout {   // the regions in workspace order
    LinkLayout(int64_t n_, int cus) : n((size_t)n_), ld((int64_t)align_up(n, 16)), g(step_grid(ld, kLkSlice, cus)) {}
    size_t n;
    int64_t ld;   // rows are ld doubles apart
    StepGrid g;   // one workgroup covers a whole number of 512-column passes
    Carver c;
    Region<LinkState> state = c.take<LinkState>(1);
    Region<int32_t> size = c.take<int32_t>((size_t)ld), chain = c.take<int32_t>((size_t)ld);
    Region<double> merges = c.take<double>(n * 4), part = c.take<double>(2 * kLkThreads), D = c.take<double>(n * (size_t)ld);
};

constexpr int64_t kLkMaxN = (int64_t)1 << 24;   // indices travel as int32 and as exact doubles

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_linkage_workspace(int64_t n, int32_t d) {
    if (n < 2 || n > kLkMaxN || d < 1 || d > kLkMaxD) return 0;
    // sized for the largest grid the driver may pick, whatever the device: the layout only depends on the CU count through
    // `per`, not through any offset
    return LinkLayout(n, kLkThreads).c.total;
}

// the matrix fill alone, into a workspace laid out as dcv_linkage lays it out (tools/linkage_bench.py times it)
extern "C" int dcv_linkage_pdist(const double* P_d, int64_t n, int32_t d, void* ws_d, size_t ws_bytes, void* stream) {
    DCV_REQUIRE(n >= 2 && n <= kLkMaxN && d >= 1 && d <= kLkMaxD && P_d, "dcv_linkage_pdist: bad arguments (n=%lld d=%d)", (long long)n, d);
    DCV_REQUIRE_POINTS_WORKSPACE("dcv_linkage_pdist", ws_d, ws_bytes, dcv_linkage_workspace(n, d));
    const LinkLayout L(n, kLkThreads);
    const int col_blocks = (int)cdiv(n, kLkSlice);
    const int64_t pd_blocks = cdiv(n, kLkPdRows) * col_blocks;
    DCV_REQUIRE(pd_blocks < ((int64_t)1 << 31), "dcv_linkage_pdist: n = %lld needs too many workgroups", (long long)n);
    hipLaunchKernelGGL(linkage_pdist_kernel, dim3((unsigned)pd_blocks), dim3(kLkThreads), 0, as_stream(stream), P_d, n, (int)d, L.ld,
                       L.D.in(ws_d), col_blocks);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

extern "C" int dcv_linkage(const double* P_d, int64_t n, int32_t d, int32_t method, double* Z_h, int64_t* searches_h, void* ws_d,
                           size_t ws_bytes, void* stream) {
    DCV_REQUIRE(n >= 2 && n <= kLkMaxN, "dcv_linkage: n = %lld, supported 2..%lld", (long long)n, (long long)kLkMaxN);
    DCV_REQUIRE(d >= 1 && d <= kLkMaxD, "dcv_linkage: d = %d, supported 1..%d", d, kLkMaxD);
    DCV_REQUIRE(method == kLkComplete || method == kLkAverage || method == kLkWard,
                "dcv_linkage: method %d (0 complete, 1 average, 2 ward)", method);
    DCV_REQUIRE(P_d && Z_h, "dcv_linkage: null points or result");
    DCV_REQUIRE_POINTS_WORKSPACE("dcv_linkage", ws_d, ws_bytes, dcv_linkage_workspace(n, d));
    DCV_REQUIRE((reinterpret_cast<uintptr_t>(ws_d) & 15) == 0, "dcv_linkage: workspace not 16-byte aligned");
    hipStream_t s = as_stream(stream);
    const LinkLayout L(n, num_cus());
    LinkState* st = L.state.in(ws_d);
    int32_t* size = L.size.in(ws_d);
    int32_t* chain = L.chain.in(ws_d);
    double* merges = L.merges.in(ws_d);

    hipLaunchKernelGGL(linkage_init_kernel, dim3((unsigned)cdiv(L.ld, 256)), dim3(256), 0, s, st, size, chain, n, L.ld);
    DCV_CHECK_LAUNCH();
    if (const int rc = dcv_linkage_pdist(P_d, n, d, ws_d, ws_bytes, stream)) return rc;

    const int64_t max_searches = 3 * (n - 1);
    const auto step = method == kLkComplete ? linkage_step_kernel<kLkComplete>
                      : method == kLkAverage ? linkage_step_kernel<kLkAverage>
                                             : linkage_step_kernel<kLkWard>;
    struct {
        int32_t merges, done, error, chain_len;
        int64_t searches;
    } h = {0, 0, 0, 1, 0};
    const int rc = run_steps(
        s, st, h, max_searches,
        [&](const auto& head, int64_t left) {
            // every merge still missing costs at least one step: a block of that many steps cannot run past the end
            int64_t steps = (int64_t)(n - 1) - head.merges;
            steps = steps < 256 ? 256 : (steps > 4096 ? 4096 : steps);
            return steps < left ? steps : left;
        },
        [&] {
            hipLaunchKernelGGL(step, dim3(L.g.grid), dim3(kLkThreads), 0, s, st, L.D.in(ws_d), size, chain, merges, L.part.in(ws_d), (int)n, L.ld,
                               L.g.per, max_searches);
        });
    if (rc) return rc;
    if (searches_h) *searches_h = h.searches;
    DCV_REQUIRE(h.error == 0 && h.done, "dcv_linkage: the chain did not finish (%s; %d of %lld merges after %lld searches): non-finite input?",
                h.error == 1 ? "a search found no candidate" : "more than 3 (n - 1) searches", h.merges, (long long)(n - 1),
                (long long)h.searches);

    std::vector<double> raw((size_t)(n - 1) * 4);
    DCV_CHECK_HIP(hipMemcpyAsync(raw.data(), merges, raw.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    // scipy: stable sort by height, then the union-find pass that names the i-th sorted merge n + i
    std::vector<int64_t> order((size_t)(n - 1));
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return raw[4 * a + 2] < raw[4 * b + 2]; });
    std::vector<int64_t> parent((size_t)(2 * n - 1));
    std::iota(parent.begin(), parent.end(), (int64_t)0);
    auto find = [&](int64_t a) {
        int64_t r = a;
        while (parent[r] != r) r = parent[r];
        while (parent[a] != r) {
            const int64_t nx = parent[a];
            parent[a] = r;
            a = nx;
        }
        return r;
    };
    for (int64_t i = 0; i < n - 1; ++i) {
        const double* z = &raw[4 * order[i]];
        const int64_t a = find((int64_t)z[0]), b = find((int64_t)z[1]);
        Z_h[4 * i + 0] = (double)(a < b ? a : b);
        Z_h[4 * i + 1] = (double)(a < b ? b : a);
        Z_h[4 * i + 2] = z[2];
        Z_h[4 * i + 3] = z[3];
        parent[a] = parent[b] = n + i;
    }
    return DCV_OK;
}

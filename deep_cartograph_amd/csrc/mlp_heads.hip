// MLP engine, loss-head unit: what lies between the network's output and its gradient -- Deep-TICA batch statistics, the
// d x d loss head, the loss gradient and the fused backward of a narrow last layer; the autoencoder's squared error and its
// gradient.  The other units reach the kernels through the host launchers at the end of the file.
#include "mlp_state.h"
#include "loss_head.h"
#include <math.h>

namespace dcv {

// ------------------------------------------------------------------ Deep-TICA batch statistics
// F: f_t of sample r in row r, f_lag in row r + lag_off, d columns (lag_off = B when the two halves
// of the batch are separate rows, = lag when a contiguous batch shares its rows: see dcv_mlp_forward).
// Each block stages kStatBlockRows pairs in
// LDS (float64) and every thread owns whole outputs of [sum f_t | sum f_lag | sum f_t f_t^T |
// sum f_t f_lag^T]; part[block][2d + 2d^2] float64, combined in block order afterwards.
__global__ __launch_bounds__(256) void tica_stats_kernel(const float* __restrict__ F, int64_t ld, int B, int d, int lag_off,
                                                         double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* s_t = reinterpret_cast<double*>(smem);   // [rows][d]
    double* s_l = s_t + kStatBlockRows * d;           // [rows][d]
    const int W = 2 * d + 2 * d * d;
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kStatBlockRows;
    const int nr = (int)(r0 + kStatBlockRows < B ? kStatBlockRows : B - r0);
    for (int i = t; i < nr * d; i += 256) {
        const int r = i / d, c = i - r * d;
        s_t[i] = (double)F[(r0 + r) * ld + c];
        s_l[i] = (double)F[(r0 + r + lag_off) * ld + c];   // lag_off = B (two halves) or lag (shared rows)
    }
    __syncthreads();
    double* my = part + (int64_t)blockIdx.x * W;
    for (int o = t; o < W; o += 256)
        my[o] = tica_stat_entry(o, d, nr, [&](int r, int i) { return s_t[r * d + i]; }, [&](int r, int i) { return s_l[r * d + i]; });
}

// out[i] = sum_b part[b][i], one wave per output, fixed combination tree
__global__ __launch_bounds__(64) void sum_partials_kernel(const double* __restrict__ part, int nblocks, int width,
                                                          double* __restrict__ out) {
    const int i = blockIdx.x;
    if (i >= width) return;
    const int lane = threadIdx.x;
    const double s = wave_sum_in_order([&](int b) { return part[(int64_t)b * width + i]; }, nblocks, lane);
    if (lane == 0) out[i] = s;
}

// One thread: C0, Ctau, loss = -tr((A Ctau)^2) with A = (C0 + reg I)^-1, and the matrices that
// turn (f_t - mu, f_lag - mu) into dL/df (see DESIGN.md "Deep-TICA gradient").  DT > 0 fixes the
// dimension at compile time (everything in registers); DT == 0 is the generic d <= 16 form.
template <int DT>
__device__ __forceinline__ void tica_grad_body(const double* __restrict__ stats, int d_rt, double Bg, double reg, double* __restrict__ gradp,
                                               double* __restrict__ log, int* __restrict__ log_count, int log_cap, int log_width) {
    constexpr int DM = DT > 0 ? DT : kMaxTicaDim;
    const int d = DT > 0 ? DT : d_rt;
    // one thread, a dependent chain: float64 divisions (a ~30-instruction sequence each) are replaced by multiplications
    // with 1 / B and the reciprocals of the Cholesky diagonal -- 1 + d divisions instead of ~8 d^2
    double mu[DM], ml[DM], invL[DM];
    double C0[DM * DM], Ct[DM * DM], A[DM * DM], K[DM * DM], T[DM * DM], Lc[DM * DM];
    const double invB = 1.0 / Bg;
    const double* sft = stats;
    const double* sfl = stats + d;
    const double* Stt = stats + 2 * d;
    const double* Stl = stats + 2 * d + d * d;
#pragma unroll
    for (int i = 0; i < DM; ++i)
        if (i < d) {
            mu[i] = sft[i] * invB;
            ml[i] = sfl[i] * invB;
        }
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j)
            if (i < d && j < d) {
                C0[i * DM + j] = 0.5 * (Stt[i * d + j] + Stt[j * d + i]) * invB - mu[i] * mu[j];
                const double cij = Stl[i * d + j] * invB - mu[i] * ml[j];
                const double cji = Stl[j * d + i] * invB - mu[j] * ml[i];
                Ct[i * DM + j] = 0.5 * (cij + cji);
            }
    // Cholesky of C0 + reg I
    bool ok = true;
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j)
            if (i < d && j <= i) {
                double s = C0[i * DM + j] + (i == j ? reg : 0.0);
#pragma unroll
                for (int k = 0; k < DM; ++k)
                    if (k < j) s -= Lc[i * DM + k] * Lc[j * DM + k];
                if (i == j) {
                    if (!(s > 0.0)) ok = false;
                    Lc[i * DM + i] = sqrt(s);
                    invL[i] = 1.0 / Lc[i * DM + i];
                } else {
                    Lc[i * DM + j] = s * invL[j];
                }
            }
    // A = (L L^T)^-1 : solve L Y = I, then L^T A = Y
#pragma unroll
    for (int c = 0; c < DM; ++c)
        if (c < d) {
            double y[DM];
#pragma unroll
            for (int i = 0; i < DM; ++i)
                if (i < d) {
                    double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
                    for (int k = 0; k < DM; ++k)
                        if (k < i) s -= Lc[i * DM + k] * y[k];
                    y[i] = s * invL[i];
                }
#pragma unroll
            for (int ii = 0; ii < DM; ++ii) {
                const int i = DM - 1 - ii;
                if (i < d) {
                    double s = y[i];
#pragma unroll
                    for (int k = 0; k < DM; ++k)
                        if (k > i && k < d) s -= Lc[k * DM + i] * A[k * DM + c];
                    A[i * DM + c] = s * invL[i];
                }
            }
        }
    // K = A Ct ; loss = -tr(K K)
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j)
            if (i < d && j < d) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < DM; ++k)
                    if (k < d) s += A[i * DM + k] * Ct[k * DM + j];
                K[i * DM + j] = s;
            }
    double loss = 0.0;
#pragma unroll
    for (int i = 0; i < DM; ++i)
#pragma unroll
        for (int j = 0; j < DM; ++j)
            if (i < d && j < d) loss -= K[i * DM + j] * K[j * DM + i];
    if (!ok) loss = NAN;
    if (gradp) {
        // T = K A  (= A Ct A, symmetric) ; Gtau = -2 T ; G0 = 2 K T
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j)
                if (i < d && j < d) {
                    double s = 0.0;
#pragma unroll
                    for (int k = 0; k < DM; ++k)
                        if (k < d) s += K[i * DM + k] * A[k * DM + j];
                    T[i * DM + j] = s;
                }
        double* g_mu = gradp;
        double* g_u = gradp + d;
        double* g_v = g_u + d * d;
        double* g_c = g_v + d * d;
#pragma unroll
        for (int i = 0; i < DM; ++i)
            if (i < d) {
                g_mu[i] = mu[i];
                double cs = 0.0;
#pragma unroll
                for (int j = 0; j < DM; ++j)
                    if (j < d) {
                        double g0 = 0.0;
#pragma unroll
                        for (int k = 0; k < DM; ++k)
                            if (k < d) g0 += K[i * DM + k] * T[k * DM + j];
                        const double Gt = -(T[i * DM + j] + T[j * DM + i]);  // -2 * sym(T)
                        g_u[i * d + j] = 4.0 * g0 * invB;                     // (2/B) G0, G0 = 2 K T
                        g_v[i * d + j] = Gt * invB;                           // (1/B) Gtau
                        cs += Gt * (ml[j] - mu[j]);
                    }
                g_c[i] = -cs * invB;
            }
    }
    const int slot = *log_count;
    if (slot < log_cap) {
        double* rec = log + (int64_t)slot * log_width;
        rec[0] = loss;
        rec[1] = Bg;
#pragma unroll
        for (int i = 0; i < DM; ++i)
#pragma unroll
            for (int j = 0; j < DM; ++j)
                if (i < d && j < d) {
                    rec[2 + i * d + j] = C0[i * DM + j];
                    rec[2 + d * d + i * d + j] = Ct[i * DM + j];
                }
#pragma unroll
        for (int i = 0; i < DM; ++i)
            if (i < d) rec[2 + 2 * d * d + i] = mu[i];
    }
    *log_count = slot + 1;
}
template <int DT>
__global__ void tica_grad_kernel(const double* __restrict__ stats, int d_rt, double Bg, double reg, double* __restrict__ gradp,
                                 double* __restrict__ log, int* __restrict__ log_count, int log_cap, int log_width) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    tica_grad_body<DT>(stats, d_rt, Bg, reg, gradp, log, log_count, log_cap, log_width);
}

typedef void (*TicaGradFn)(const double*, int, double, double, double*, double*, int*, int, int);
// (d <= 4 takes the wave form below; <0>: every other dimension)
static TicaGradFn tica_grad_fn(int d) { return d == 5 ? tica_grad_kernel<5> : d == 6 ? tica_grad_kernel<6> : tica_grad_kernel<0>; }

// the wave-parallel loss head as a launch of its own: the data-parallel path, where the batch statistics are all-reduced
// between the statistics kernel and the head (the single-thread form above is a chain of ~2000 dependent float64
// instructions, 8 us; this one ~3 us)
template <int D>
__global__ __launch_bounds__(64) void tica_grad_wave_kernel(const double* __restrict__ stats, double Bg, double reg, double* __restrict__ gradp,
                                                            double* __restrict__ log, int* __restrict__ log_count, int log_cap, int log_width) {
    __shared__ TicaWaveLds<D> s_head;
    __shared__ double s_stats[2 * D + 2 * D * D];
    if (threadIdx.x < 2 * D + 2 * D * D) s_stats[threadIdx.x] = stats[threadIdx.x];
    wave_sync_lds();
    tica_grad_wave<D>(s_head, s_stats, Bg, reg, gradp, log, log_count, log_cap, log_width, (int)threadIdx.x);
}
typedef void (*TicaGradWaveFn)(const double*, double, double, double*, double*, int*, int, int);
static TicaGradWaveFn tica_grad_wave_fn(int d) {
    static const TicaGradWaveFn fn[] = {   // by dimension; [0]: every other one
        nullptr, tica_grad_wave_kernel<1>, tica_grad_wave_kernel<2>, tica_grad_wave_kernel<3>, tica_grad_wave_kernel<4>};
    return fn[d >= 1 && d <= 4 ? d : 0];
}

// The same statistics for D <= 4 outputs with every thread at work: a thread walks whole rows (its pair's
// 2 D values, 2 D + 2 D^2 float64 accumulators in registers), waves combine by shuffles, the block through
// LDS.  rows_per_block pairs per block (a multiple of 256; stats_plan): enough blocks to spread a small batch over
// the chip, few enough partials for the last block's ordered sum.  One launch: the block that finishes last adds the
// partials up in block order and -- on one GPU, where nothing is all-reduced in between (fused.on) -- goes straight
// on to the d x d loss head (tica_grad_wave, on its wave 0), saving the launch of tica_grad_wave_kernel.
// GROUP: member `member` of `members` batches evaluated side by side (tica_stats_rows_group_kernel): the caller hands in the
// member's own rows, partials and ticket; its record goes to slot (counter + member) (loss_head.h: log_member), the counter
// stays put until launch_log_advance behind the launch.
template <int D, bool GROUP>
__device__ __forceinline__ void tica_stats_rows_body(const float* __restrict__ F, int64_t ld, int B, int lag_off, int rows_per_block,
                                                     double* __restrict__ part, unsigned* __restrict__ ticket, double* __restrict__ out,
                                                     const FusedHead& fused, int member, int members) {
    constexpr int W = 2 * D + 2 * D * D;
    __shared__ double red[4][W];
    __shared__ TicaWaveLds<D> s_head;
    __shared__ unsigned s_last;
    __shared__ int s_slot;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    double acc[W];
#pragma unroll
    for (int o = 0; o < W; ++o) acc[o] = 0.0;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < B ? r0 + rows_per_block : B;
    for (int64_t r = r0 + t; r < r1; r += 256) {
        double a[D], b[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            a[i] = (double)F[r * ld + i];
            b[i] = (double)F[(r + lag_off) * ld + i];
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            acc[i] += a[i];
            acc[D + i] += b[i];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                acc[2 * D + i * D + j] += a[i] * a[j];
                acc[2 * D + D * D + i * D + j] += a[i] * b[j];
            }
        }
    }
    // wave reduction as a butterfly reduce-scatter: every step halves the values a lane carries (W = 40 -> 20 -> 10 -> 5,
    // then three all-reduce steps): ~50 float64 shuffles per lane in independent chains instead of 6 W = 240 dependent
    // ones (a float64 shuffle is two ds_bpermute round trips: the plain form spent 14 us of latency here)
    {
        int base = 0, dup = 0;
        const int cnt = butterfly_sum<W, 32, W, double>(acc, lane, base, dup);
        if ((lane & dup) == 0) {
#pragma unroll
            for (int i = 0; i < W; ++i)
                if (i < cnt) red[wave][base + i] = acc[i];
        }
    }
    __syncthreads();
    if (t < W) handoff_store(part + (int64_t)blockIdx.x * W + t, ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]);
    // the block that finishes last adds the partials up in block order (no second launch; same sums whichever
    // block it is).  Hand-off between the blocks: handoff.h (write-through partials, drained by every wave before the
    // barrier and the agent-scope ticket; the last arriver acquires at agent scope and reads with sc1 loads).
    if (handoff_arrive_last(ticket, gridDim.x, &s_last)) {
        constexpr int G = 256 / W;
        __shared__ double s_grp[G * W];
        const double s = block_sum_partials_in_order(part, gridDim.x, W, G, t, s_grp);
        if (t < W) {
            if (!GROUP || member == members - 1) out[t] = s;   // (a group leaves the statistics of its last batch, as stepping does)
            red[0][t] = s;
        }
        if (fused.on) {
            __syncthreads();
            if (wave == 0) {
                if constexpr (!GROUP) {
                    tica_grad_wave<D>(s_head, &red[0][0], fused.Bg, fused.reg, fused.gradp, fused.log, fused.log_count, fused.log_cap, fused.log_width, lane);
                } else {
                    // records in batch order (loss_head.h: log_member): the head moves a private copy of the counter only
                    if (lane == 0) s_slot = *fused.log_count;
                    wave_sync_lds();
                    const MemberLog ml = log_member(fused.log, fused.log_width, fused.log_cap, member);
                    tica_grad_wave<D>(s_head, &red[0][0], fused.Bg, fused.reg, fused.gradp, ml.log, &s_slot, ml.cap, fused.log_width, lane);
                }
            }
        }
    }
}
template <int D>
__global__ __launch_bounds__(256) void tica_stats_rows_kernel(const float* __restrict__ F, int64_t ld, int B, int lag_off,
                                                              int rows_per_block, double* __restrict__ part, unsigned* __restrict__ ticket,
                                                              double* __restrict__ out, FusedHead fused) {
    tica_stats_rows_body<D, false>(F, ld, B, lag_off, rows_per_block, part, ticket, out, fused, 0, 1);
}
// blockIdx.y = member: the network outputs of member j begin f_stride floats behind member j - 1's, its partials are
// part + j * gridDim.x * W, its ticket is ticket[j] (zero between launches)
template <int D>
__global__ __launch_bounds__(256) void tica_stats_rows_group_kernel(const float* __restrict__ F, int64_t ld, int64_t f_stride, int B, int lag_off,
                                                                    int rows_per_block, double* __restrict__ part, unsigned* __restrict__ ticket,
                                                                    double* __restrict__ out, FusedHead fused) {
    constexpr int W = 2 * D + 2 * D * D;
    const int j = blockIdx.y, n = gridDim.y;
    tica_stats_rows_body<D, true>(F + (int64_t)j * f_stride, ld, B, lag_off, rows_per_block, part + (int64_t)j * gridDim.x * W, ticket + j, out, fused, j, n);
}
// the log counter behind a batched launch whose members only read it (loss_head.h: log_member): + n records
__global__ void log_advance_kernel(int* __restrict__ log_count, int n) { *log_count += n; }
typedef void (*tica_stats_fn_t)(const float*, int64_t, int, int, int, double*, unsigned*, double*, FusedHead);
static tica_stats_fn_t tica_stats_rows_fn(int d) {
    static const tica_stats_fn_t fn[] = {   // by dimension; [0]: every other one
        nullptr, tica_stats_rows_kernel<1>, tica_stats_rows_kernel<2>, tica_stats_rows_kernel<3>, tica_stats_rows_kernel<4>};
    return fn[d >= 1 && d <= 4 ? d : 0];
}
typedef void (*tica_stats_group_fn_t)(const float*, int64_t, int64_t, int, int, int, double*, unsigned*, double*, FusedHead);
static tica_stats_group_fn_t tica_stats_rows_group_fn(int d) {
    static const tica_stats_group_fn_t fn[] = {   // by dimension; [0]: every other one
        nullptr, tica_stats_rows_group_kernel<1>, tica_stats_rows_group_kernel<2>, tica_stats_rows_group_kernel<3>,
        tica_stats_rows_group_kernel<4>};
    return fn[d >= 1 && d <= 4 ? d : 0];
}
// rows per block of the kernels above: at most 512 blocks, whole multiples of 256 rows
int stats_rows_per_block(int64_t batch) { return (int)(cdiv(cdiv(batch, 256), 256) * 256); }   // <= 256 blocks: each ends on one ticket (~70 ns apiece, serialised)

// Gradient of the loss w.r.t. the network outputs (loss_head.h: tica_grad_t / tica_grad_l, and why float64).  Sample i
// (0 <= i < B) has f_t in row i and f_lag in row i + lag_off.  Row j of dZ collects whatever lands on it: its own
// t-gradient (j < B) plus the lag-gradient of sample j - lag_off (j >= lag_off).  With lag_off = B the halves are
// disjoint; with lag_off = lag (contiguous batch, shared rows) an interior row receives both.  Multiplied by act'(F) of
// the last layer.
__global__ __launch_bounds__(256) void tica_dF_kernel(const float* __restrict__ F, int64_t ldf, int B, int d, int lag_off,
                                                      const double* __restrict__ gradp, int act, float* __restrict__ dZ,
                                                      int64_t ldz, DropCfg drop, float hscale) {
    __shared__ double s_g[kMaxTicaDim * (2 * kMaxTicaDim + 2)];
    const int np = d + 2 * d * d + d;
    for (int i = threadIdx.x; i < np; i += 256) s_g[i] = gradp[i];
    __syncthreads();
    const TicaGradMats G = tica_grad_mats(s_g, d);
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t rows = (int64_t)B + lag_off;
    if (j >= rows) return;
    const bool has_t = j < B;            // row j is the f_t row of sample j
    const bool has_l = j >= lag_off;     // row j is the f_lag row of sample j - lag_off
    float fj[kMaxTicaDim], fv[kMaxTicaDim], fw[kMaxTicaDim];
    for (int i = 0; i < d; ++i) {
        fj[i] = F[j * ldf + i];
        fv[i] = has_t ? F[(j + lag_off) * ldf + i] : 0.f;   // f_lag of sample j
        fw[i] = has_l ? F[(j - lag_off) * ldf + i] : 0.f;   // f_t of sample j - lag_off
    }
    for (int i = 0; i < d; ++i) {
        double g = has_t ? tica_grad_t<0>(i, d, G.mu, G.Gu, G.Gv, G.c, fj, fv) : 0.0;
        if (has_l) g += tica_grad_l<0>(i, d, G.mu, G.Gv, fw);
        float gf = (float)g;
        if (drop.thr != 0u) gf *= f4c(drop.mult(j, i & ~3), i & 3);   // F holds act(z) * keep / (1 - p)
        dZ[j * ldz + i] = gf * act_grad_from_out(act, fj[i] * hscale);
    }
}

// ------------------------------------------------------------------ fused backward of a narrow last layer
// Deep-TICA's last Linear maps K hidden units to D <= 8 outputs: as separate products its wgrad, dgrad and the
// two bias-gradient passes each stream the K-wide activations H (or write the K-wide dZ) for a handful of
// flops per byte.  One pass does all of it: per row r
//   g      = dL/dz_last[r]  (D values; the gradient row of tica_dF_kernel, evaluated in place)
//   dW    += g (x) H[r]          -> slab[block][D][K]          (wgrad partial of the last layer)
//   db    += g                   -> bpart_last[block][D]
//   dZ[r]  = (g W) * act'(H[r])  -> written once, 16-byte stores (dgrad of the last layer)
//   db'   += dZ[r]               -> bpart_prev[block][K]       (bias gradient of the layer before)
// HBM: K floats read + K floats written per row.  Thread (row group rl, 4 columns c4): D x 4 weights and
// D x 4 + 4 accumulators in registers; the 256 / (K/4) row groups of a block are combined through LDS in
// fixed order, blocks by reduce_grads_kernel in float64.
template <int D>
__global__ __launch_bounds__(256) void head_backward_kernel(const float* __restrict__ F, int64_t ldf, int B, int lag_off,
                                                            const double* __restrict__ gradp, int act_last,
                                                            const float* __restrict__ H, int64_t ldh, int K, int act_prev,
                                                            const float* __restrict__ W, int64_t rows_per_block,
                                                            float* __restrict__ dZ, int64_t ldz, float* __restrict__ slab,
                                                            float* __restrict__ bpart_last, float* __restrict__ bpart_prev,
                                                            DropCfg drop_prev, float hscale_prev) {
    constexpr int U = 4;                        // rows in flight per thread
    extern __shared__ __attribute__((aligned(16))) double s_memd[];
    double* s_g = s_memd;                       // mu | Gu | Gv | c   (float64: loss_head.h)
    float* s_gf = reinterpret_cast<float*>(s_memd + (2 * D + 2 * D * D));  // [groups][U][D] loss gradients of the rows in flight
    const int t = threadIdx.x;
    const int C4 = K / 4, groups = 256 / C4;    // a row group (C4 <= 64 lanes) lies inside one wave
    float* s_red = s_gf + groups * U * D;       // [groups][(D + 1) * K + D]
    for (int i = t; i < 2 * D + 2 * D * D; i += 256) s_g[i] = gradp[i];
    __syncthreads();
    const TicaGradMats G = tica_grad_mats(s_g, D);
    const int c4 = t % C4, rl = t / C4;
    const int64_t rows = (int64_t)B + lag_off;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float4 w[D], aw[D];
    float4 ab = make_float4(0.f, 0.f, 0.f, 0.f);
    float al[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        w[j] = *reinterpret_cast<const float4*>(W + (int64_t)j * K + c4 * 4);
        aw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        al[j] = 0.f;
    }
    float* gmine = s_gf + rl * U * D;
    for (int64_t rb = r0 + rl; rb < r1; rb += (int64_t)groups * U) {
        float4 h[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {   // the K-wide loads first: U rows in flight
            const int64_t r = rb + (int64_t)q * groups;
            h[q] = r < r1 ? *reinterpret_cast<const float4*>(H + r * ldh + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // dL/dz_last of the U rows: component i by lane i, i + C4, ... of the row group, shared through LDS.  The output
        // rows it needs (own row, the pair's lagged row, the row it is the lagged row of) are loaded up front, unconditionally
        // and for all U rows at once, from clamped row indices: inside the has_t / has_l branches they were two dependent
        // round trips per row (9.0 -> 8.3 us at 8202 rows; large batch 181 -> 185 M frames/s).
        float fro[U][D], fvo[U][D], fwo[U][D];
        if (c4 < D) {
            const bool fvec = D == 4 && (ldf & 3) == 0 && (reinterpret_cast<uintptr_t>(F) & 15) == 0;
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int64_t r = rb + (int64_t)q * groups;
                const int64_t rt = r < r1 ? r : r0;                          // a row of this block (not used when r >= r1)
                const int64_t rv = (r < r1 && r < B) ? r + lag_off : rt;     // < B + lag_off = rows
                const int64_t rw = (r < r1 && r >= lag_off) ? r - lag_off : rt;
                if constexpr (D == 4) {
                    if (fvec) {
                        const float4 x = *reinterpret_cast<const float4*>(F + rt * ldf);
                        const float4 y = *reinterpret_cast<const float4*>(F + rv * ldf);
                        const float4 z = *reinterpret_cast<const float4*>(F + rw * ldf);
                        fro[q][0] = x.x; fro[q][1] = x.y; fro[q][2] = x.z; fro[q][3] = x.w;
                        fvo[q][0] = y.x; fvo[q][1] = y.y; fvo[q][2] = y.z; fvo[q][3] = y.w;
                        fwo[q][0] = z.x; fwo[q][1] = z.y; fwo[q][2] = z.z; fwo[q][3] = z.w;
                        continue;
                    }
                }
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    fro[q][k] = F[rt * ldf + k];
                    fvo[q][k] = F[rv * ldf + k];
                    fwo[q][k] = F[rw * ldf + k];
                }
            }
        }
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t r = rb + (int64_t)q * groups;
            for (int i = c4; i < D; i += C4) {
                float gi = 0.f;
                if (r < r1) {
                    const bool has_t = r < B, has_l = r >= lag_off;
                    double gd = has_t ? tica_grad_t<D>(i, D, G.mu, G.Gu, G.Gv, G.c, fro[q], fvo[q]) : 0.0;
                    if (has_l) gd += tica_grad_l<D>(i, D, G.mu, G.Gv, fwo[q]);
                    gi = (float)gd * act_grad_from_out(act_last, pick(i, fro[q]));
                }
                gmine[q * D + i] = gi;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t r = rb + (int64_t)q * groups;
            if (r >= r1) break;
            float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const float g = gmine[q * D + j];
                z.x = fmaf(g, w[j].x, z.x); z.y = fmaf(g, w[j].y, z.y); z.z = fmaf(g, w[j].z, z.z); z.w = fmaf(g, w[j].w, z.w);
                aw[j].x = fmaf(g, h[q].x, aw[j].x); aw[j].y = fmaf(g, h[q].y, aw[j].y);
                aw[j].z = fmaf(g, h[q].z, aw[j].z); aw[j].w = fmaf(g, h[q].w, aw[j].w);
                if (c4 == 0) al[j] += g;
            }
            z.x *= act_grad_from_out(act_prev, h[q].x * hscale_prev); z.y *= act_grad_from_out(act_prev, h[q].y * hscale_prev);
            z.z *= act_grad_from_out(act_prev, h[q].z * hscale_prev); z.w *= act_grad_from_out(act_prev, h[q].w * hscale_prev);
            if (drop_prev.thr != 0u) {   // H holds act(z) * keep / (1 - p): the same mask scales the gradient
                const float4 k = drop_prev.mult(r, c4 * 4);
                z.x *= k.x; z.y *= k.y; z.z *= k.z; z.w *= k.w;
            }
            handoff_store16(dZ + r * ldz + c4 * 4, hv4f{z.x, z.y, z.z, z.w});   // write-through: nothing to write back when the launch ends
            ab.x += z.x; ab.y += z.y; ab.z += z.z; ab.w += z.w;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();   // gmine is rewritten by the next iteration
    }
    // combine the row groups: s_red[rl] = [dW (D x K) | db' (K) | db (D)]
    const int stride = (D + 1) * K + D;
    float* mine = s_red + (int64_t)rl * stride;
#pragma unroll
    for (int j = 0; j < D; ++j) *reinterpret_cast<float4*>(mine + j * K + c4 * 4) = aw[j];
    *reinterpret_cast<float4*>(mine + D * K + c4 * 4) = ab;
    if (c4 == 0) {
#pragma unroll
        for (int j = 0; j < D; ++j) mine[(D + 1) * K + j] = al[j];
    }
    __syncthreads();
    for (int i = t; i < stride; i += 256) {
        float tot = 0.f;
        for (int q = 0; q < groups; ++q) tot += s_red[(int64_t)q * stride + i];
        if (i < D * K) slab[(int64_t)blockIdx.x * D * K + i] = tot;
        else if (i < (D + 1) * K) bpart_prev[(int64_t)blockIdx.x * K + (i - D * K)] = tot;
        else bpart_last[(int64_t)blockIdx.x * D + (i - (D + 1) * K)] = tot;
    }
}

typedef void (*head_backward_fn_t)(const float*, int64_t, int, int, const double*, int, const float*, int64_t, int, int, const float*, int64_t,
                                   float*, int64_t, float*, float*, float*, DropCfg, float);
static head_backward_fn_t head_backward_fn(int d) {
    static const head_backward_fn_t fn[] = {   // by dimension; [0]: every other one
        nullptr, head_backward_kernel<1>, head_backward_kernel<2>, head_backward_kernel<3>, head_backward_kernel<4>,
        head_backward_kernel<5>, head_backward_kernel<6>, head_backward_kernel<7>, head_backward_kernel<8>};
    return fn[d >= 1 && d <= 8 ? d : 0];
}

// ------------------------------------------------------------------ autoencoder loss
// SSE = sum ((y - xn) * range)^2 over rows x F ; part[block]
// `ticket` != null: the last block to finish adds the partials up in block order (the sum sum_partials_kernel would
// produce) into out[0] and, when `log` != null, appends the step's loss record (ae_log_kernel) -- the one-GPU step
// then needs neither of those two launches.
__global__ __launch_bounds__(256) void ae_sse_kernel(const float* __restrict__ Y, int64_t ldy, const float* __restrict__ Xn,
                                                     int64_t ldx, RowMap rows, int64_t R, int F,
                                                     const float* __restrict__ range, double* __restrict__ part,
                                                     unsigned* __restrict__ ticket, double* __restrict__ out, double Bg,
                                                     double* __restrict__ log, int* __restrict__ log_count, int log_cap,
                                                     int log_width, int rows_per_block, const double* __restrict__ kpart = nullptr,
                                                     int kblocks = 0, double beta = 0.0) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < R ? r0 + rows_per_block : R;
    // the block's rows x F elements flat over the threads, eight independent element loads in flight per thread
    // (a thread that walked its rows one after the other spent the kernel waiting: 16 dependent round trips, 27 us)
    double s = 0.0;
    const int per_block = (int)(r1 - r0) * F;
    for (int e0 = t; e0 < per_block; e0 += 8 * 256) {
        float ev[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + 256 * u;
            ev[u] = 0.f;
            if (e < per_block) {
                const int rr = e / F, c = e - rr * F;
                const int64_t r = r0 + rr;
                ev[u] = (Y[r * ldy + c] - Xn[rows.template get<true>(r) * ldx + c]) * range[c];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)ev[u] * (double)ev[u];
    }
    red[t] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (ticket == nullptr) {
        if (t == 0) part[blockIdx.x] = red[0];
        return;
    }
    if (t == 0) handoff_store(part + blockIdx.x, red[0]);
    __shared__ unsigned is_last;
    if (!handoff_arrive_last(ticket, gridDim.x, &is_last)) return;   // handoff.h; see tica_stats_rows_kernel
    if (t < 64) {   // one wave, the sum sum_partials_kernel would produce
        const double tot = wave_sum_in_order([&](int b) { return handoff_load(part + b); }, (int)gridDim.x, t);
        double kl = 0.0;   // VAE: the KL partials of the sampling launch (vae_sample_kernel: an earlier launch, plain loads)
        if (kpart != nullptr) kl = wave_sum_in_order([&](int b) { return kpart[b]; }, kblocks, t);
        if (t == 0) {
            out[0] = tot;
            if (kpart != nullptr) out[1] = kl;
            if (log != nullptr) {
                const int slot = *log_count;
                if (slot < log_cap) ae_loss_record(log + (int64_t)slot * log_width, tot, kl, Bg, F, beta, kpart != nullptr);
                *log_count = slot + 1;
            }
        }
    }
}

// dY = scale * (y - xn) * range^2 * act'(y)
__global__ __launch_bounds__(256) void ae_dY_kernel(const float* __restrict__ Y, int64_t ldy, const float* __restrict__ Xn,
                                                    int64_t ldx, RowMap rows, int64_t R, int F,
                                                    const float* __restrict__ range, float scale, int act,
                                                    float* __restrict__ dZ, int64_t ldz, DropCfg drop, float hscale) {
    const int64_t total = R * F;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / F;
        const int c = (int)(i - r * F);
        const float y = Y[r * ldy + c];
        const float x = Xn[rows.template get<true>(r) * ldx + c];
        const float rg = range[c];
        float g = scale * (y - x) * rg * rg * act_grad_from_out(act, y * hscale);
        if (drop.thr != 0u) g *= f4c(drop.mult(r, c & ~3), c & 3);
        dZ[r * ldz + c] = g;
    }
}

// vae != 0: stats = [SSE | KL sum], record [recon + beta * kl | weight | recon | kl]
__global__ void ae_log_kernel(const double* __restrict__ stats, double Bg, int F, double* __restrict__ log,
                              int* __restrict__ log_count, int log_cap, int log_width, int vae = 0, double beta = 0.0) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int slot = *log_count;
    if (slot < log_cap) ae_loss_record(log + (int64_t)slot * log_width, stats[0], vae ? stats[1] : 0.0, Bg, F, beta, vae != 0);
    *log_count = slot + 1;
}

// the fused backward of the last layer applies to a Deep-TICA network whose last Linear is narrow (<= 8 outputs)
// and whose input width tiles a 256-thread block in 16-byte segments
static size_t head_lds_bytes(int D, int K) {
    const int groups = 256 / (K / 4);
    return (size_t)(2 * D + 2 * D * D) * sizeof(double) + ((size_t)groups * 4 * D + (size_t)groups * ((size_t)(D + 1) * K + D)) * sizeof(float);
}
bool head_fusable(const dcv_mlp* m) {
    if (head_fusion_off() || m->L < 2 || m->any_bn) return false;
    if (m->desc.dropout[m->L - 1] > 0.f) return false;   // dropout on the network output: general kernels
    const LayerPlan& p = m->layers[m->L - 1];
    const LayerPlan& q = m->layers[m->L - 2];
    const int K = p.in;
    if (p.out > 8 || K % 4 != 0 || K / 4 > 256 || 256 % (K / 4) != 0) return false;
    if (!quad_ok(q.H, q.ldh) || !quad_ok(m->dZ[0], m->ld_dz) || !quad_ok(m->dZ[1], m->ld_dz) || !quad_ok(m->params + p.w_off, K)) return false;
    if (K / 4 > 64) return false;   // a row group must lie inside one wave
    return head_lds_bytes(p.out, K) <= 60 * 1024;
}
// blocks of the fused pass: about four per CU, at least 32 rows each, bounded by the partial buffers
static void head_plan(const dcv_mlp* m, int64_t R, int64_t* rows_per_block, int64_t* blocks) {
    const LayerPlan& p = m->layers[m->L - 1];
    int64_t want = 4 * (int64_t)num_cus();
    if (want > p.max_splits) want = p.max_splits;
    int64_t rpb = cdiv(cdiv(R, want), 32) * 32;
    if (rpb < 32) rpb = 32;
    *rows_per_block = rpb;
    *blocks = cdiv(R, rpb);
}

// ------------------------------------------------------------------ host launchers: how the other units reach the kernels above
static int launched() {
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
int launch_log_advance(int* log_count, int n, hipStream_t s) {
    hipLaunchKernelGGL(log_advance_kernel, dim3(1), dim3(1), 0, s, log_count, n);
    return launched();
}
int launch_sum_partials(const double* part, int nblocks, int width, double* out, hipStream_t s) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3(width), dim3(64), 0, s, part, nblocks, width, out);
    return launched();
}
// Batch statistics of the network outputs F -> m->stats.  D <= 4: one launch; with fuse_head (forward_impl) its last block
// goes on to the loss head, and *head_ran says so.  Wider outputs: the generic kernel and the sum of its partials.
int tica_stats(dcv_mlp* m, const float* F, int64_t ldf, int batch, int lag_off, int fuse_head, bool* head_ran, hipStream_t s) {
    *head_ran = false;
    if (tica_stats_fn_t fast = tica_stats_rows_fn(m->d_out)) {
        const int rpb = stats_rows_per_block(batch);
        FusedHead fh{0, 0.0, 0.0, nullptr, nullptr, nullptr, 0, 0};
        if (fuse_head) fh = FusedHead{1, (double)batch, m->desc.tica_reg, fuse_head == 1 ? m->gradp : nullptr, m->log, m->log_count, m->log_cap, m->log_width};
        hipLaunchKernelGGL(fast, dim3((int)cdiv(batch, rpb)), dim3(256), 0, s, F, ldf, batch, lag_off, rpb, m->spart, m->ticket, m->stats, fh);
        *head_ran = fuse_head != 0;
        return launched();
    }
    const int nb = (int)cdiv(batch, kStatBlockRows);
    hipLaunchKernelGGL(tica_stats_kernel, dim3(nb), dim3(256), (size_t)2 * kStatBlockRows * m->d_out * sizeof(double), s, F, ldf, batch, m->d_out, lag_off,
                       m->spart);
    DCV_CHECK_LAUNCH();
    return launch_sum_partials(m->spart, nb, m->stats_len, m->stats, s);
}
// the same for `members` batches side by side (eval_group): member j reads F + j * f_stride and leaves record j behind the counter
bool tica_stats_groupable(int d) { return tica_stats_rows_group_fn(d) != nullptr; }
int tica_stats_group(dcv_mlp* m, const float* F, int64_t ldf, int64_t f_stride, int batch, int lag_off, int blocks, int members, double* part,
                     unsigned* tickets, hipStream_t s) {
    const FusedHead fh{1, (double)batch, m->desc.tica_reg, nullptr, m->log, m->log_count, m->log_cap, m->log_width};
    hipLaunchKernelGGL(tica_stats_rows_group_fn(m->d_out), dim3((unsigned)blocks, (unsigned)members), dim3(256), 0, s, F, ldf, f_stride, batch, lag_off,
                       stats_rows_per_block(batch), part, tickets, m->stats, fh);
    DCV_CHECK_LAUNCH();
    return launch_log_advance(m->log_count, members, s);
}
// The step's loss record from m->stats, unless the forward's launch wrote it (head_done) or the fused backward will
// (head_in_bwd).  Deep-TICA: the loss head as a launch of its own, which for a training step also leaves the matrices m->gradp.
int loss_record(dcv_mlp* m, int64_t global_batch, bool train, bool head_in_bwd, hipStream_t s) {
    if (!m->head_done && !head_in_bwd) {
        double* gradp = train ? m->gradp : nullptr;
        if (m->desc.model != DCV_MODEL_DEEPTICA) {
            hipLaunchKernelGGL(ae_log_kernel, dim3(1), dim3(64), 0, s, m->stats, (double)global_batch, m->desc.dims[0], m->log, m->log_count, m->log_cap,
                               m->log_width, m->vae_d > 0 ? 1 : 0, m->kl_beta);
        } else if (TicaGradWaveFn wf = tica_grad_wave_fn(m->d_out)) {
            hipLaunchKernelGGL(wf, dim3(1), dim3(64), 0, s, (const double*)m->stats, (double)global_batch, m->desc.tica_reg, gradp, m->log, m->log_count,
                               m->log_cap, m->log_width);
        } else {
            hipLaunchKernelGGL(tica_grad_fn(m->d_out), dim3(1), dim3(64), 0, s, m->stats, m->d_out, (double)global_batch, m->desc.tica_reg, gradp, m->log,
                               m->log_count, m->log_cap, m->log_width);
        }
        DCV_CHECK_LAUNCH();
    }
    m->head_done = false;
    return DCV_OK;
}
// loss gradient, both bias gradients, wgrad and dgrad of the narrow last layer (head_fusable) in one pass over H_{L-2}: the
// gradient of layer L - 2 into dZ, the partials into the two layers' buffers, *blocks of them
int head_backward(dcv_mlp* m, int64_t R, int batch, int lag_off, float* dZ, int* blocks, hipStream_t s) {
    const LayerPlan& p = m->layers[m->L - 1];
    const LayerPlan& q = m->layers[m->L - 2];
    const int D = p.out, K = p.in;
    int64_t rpb, nb;
    head_plan(m, R, &rpb, &nb);
    hipLaunchKernelGGL(head_backward_fn(D), dim3((unsigned)nb), dim3(256), head_lds_bytes(D, K), s, (const float*)p.H, p.ldh, batch, lag_off,
                       (const double*)m->gradp, p.act, (const float*)q.H, q.ldh, K, q.act, (const float*)(m->params + p.w_off), rpb, dZ, m->ld_dz, p.slab,
                       p.bpart, q.bpart, drop_cfg(m, m->L - 2), drop_hscale(m, m->L - 2));
    *blocks = (int)nb;
    return launched();
}
// Autoencoder: squared error of the output Y against the R input rows -> m->stats.  fuse_head (one-GPU step): final sum and loss
// record in the last block of the same launch; else the partials are summed by launches of their own ([SSE | KL sum]).
int ae_sse(dcv_mlp* m, const float* Y, int64_t ldy, const float* Xn, int64_t ldx, const RowMap& rm, int64_t R, int batch, bool fuse_head, hipStream_t s) {
    // Two opposing costs: every block ends on a release fence + ticket (~70 ns apiece, serialised: 1024 blocks measured
    // 81 us for a 2 MB pass), and every 8 elements per thread are one more round trip of loads (64 blocks x 32 elements
    // per thread measured 27 us at 4096 x 128).  16 elements per thread, at most 128 blocks up to 4M elements, then
    // 64 elements per thread up to 512 blocks; never fewer than kSseRows rows per block.
    const int64_t elems = R * (int64_t)m->desc.dims[0];
    int64_t want = cdiv(elems, 256 * 16);
    if (want > 128) want = cdiv(elems, 256 * 64) > 128 ? cdiv(elems, 256 * 64) : 128;
    if (want > 512) want = 512;
    if (want < 1) want = 1;
    int64_t rpb = cdiv(R, want);
    if (rpb < kSseRows) rpb = kSseRows;
    const int nb = (int)cdiv(R, rpb);
    // (without a ticket the kernel stops at its partial and reads none of the arguments behind it)
    hipLaunchKernelGGL(ae_sse_kernel, dim3(nb), dim3(256), 0, s, Y, ldy, Xn, ldx, rm, R, m->desc.dims[0], m->feat_range, m->spart,
                       fuse_head ? m->ticket : (unsigned*)nullptr, m->stats, (double)batch, m->log, m->log_count, m->log_cap, m->log_width, (int)rpb,
                       (const double*)(m->vae_d > 0 ? m->vae_kpart : nullptr), m->vae_kblocks, m->kl_beta);
    DCV_CHECK_LAUNCH();
    if (fuse_head) return DCV_OK;
    const int rc = launch_sum_partials(m->spart, nb, 1, m->stats, s);
    if (rc || m->vae_d == 0) return rc;
    return launch_sum_partials(m->vae_kpart, m->vae_kblocks, 1, m->stats + 1, s);
}
// dL/dz of the last layer -> dZ: the loss gradient w.r.t. the network output Y, times act'(Y) and the dropout mask of that layer
int loss_gradient(dcv_mlp* m, const float* Y, int64_t ldy, const float* Xn, int64_t ldx, const RowMap& rm, int64_t R, int batch, int lag_off,
                  int64_t global_batch, int act, float* dZ, const DropCfg& drop, float hscale, hipStream_t s) {
    if (m->desc.model == DCV_MODEL_DEEPTICA) {   // (R = batch + lag_off)
        hipLaunchKernelGGL(tica_dF_kernel, dim3((unsigned)cdiv(R, 256)), dim3(256), 0, s, Y, ldy, batch, m->d_out, lag_off, m->gradp, act, dZ, m->ld_dz, drop,
                           hscale);
        return launched();
    }
    const int F = m->desc.dims[0];
    const float scale = (float)(2.0 / ((double)global_batch * (double)F));
    int64_t blocks = cdiv(R * F, 256);
    const int64_t cap = (int64_t)num_cus() * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(ae_dY_kernel, dim3((unsigned)blocks), dim3(256), 0, s, Y, ldy, Xn, ldx, rm, R, F, m->feat_range, scale, act, dZ, m->ld_dz, drop, hscale);
    return launched();
}

}  // namespace dcv

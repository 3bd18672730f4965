// Fused Deep-TICA step of a SMALL network (the reference's own sizes: cv_calculator.py:2569-2590 builds 54-16-8-2 in its
// test configuration, F-15-15-d from tools/train_colvars/default_config.yml): every weight resident in one CU's LDS, as in
// snet.hip -- but the Deep-TICA loss couples ALL samples of the batch (the d x d covariances of the network outputs), so
// one grid-wide dependency sits between the forward and the backward pass.  A kernel boundary is the cheapest grid-wide
// synchronisation on this part: the step is TWO fused launches plus the gradient reduction,
//
//   snet_dt_fwd_kernel   a workgroup takes TR / 2 PAIRS: rows [0, TR/2) of its tile are the x_t rows, rows [TR/2, TR) the
//                        x_lag rows of the same pairs (gathered through the RowMap: contiguous, gathered and two-half
//                        batches alike) -- both halves of a pair in ONE tile, so the 2d + 2d^2 batch statistics of its
//                        pairs are formed from LDS.  Forward chain with the activations kept in LDS; statistics partial
//                        (float64, pair order); the tile's activations leave as one contiguous blob (write-through); the
//                        ticketed last arriver (handoff.h) adds the partials in block order and -- one-GPU steps -- runs
//                        the wave-parallel d x d loss head (loss_head.h).  An evaluation step ends here.
//   snet_dt_bwd_kernel   stages the weights of layers >= 1 (the input gradients need them) and its blob back into LDS,
//                        evaluates the loss gradient of its pairs in float64 from the head's matrices (loss_head.h:
//                        tica_grad_t / tica_grad_l), walks back through the layers as snet_ae_kernel does and
//                        leaves one gradient partial per workgroup and layer for reduce_grads_quad_kernel + the optimiser.
//
// Three launches instead of eight for a 3-layer network, none of them a matrix product over a few thousand rows on 516
// workgroups.  Row sharing is given up: a contiguous batch evaluates 2 B rows instead of B + lag -- at these
// widths the step is latency, not flops.  A data-parallel step uses the same two kernels with the head left to
// tica_grad_wave_kernel behind the statistics all-reduce.  Not taken (the layer-by-layer path runs): d > 4, dropout, batch
// normalisation, a width above 256, a network that does not fit in LDS, more than 512 tiles (DCV_NO_SNET=1 forces it off).
#include "snet.h"
#include "loss_head.h"
#include <new>

namespace dcv {

struct SnetDtArgs {
    SnetLayer l[DCV_MAX_LAYERS];
    int L;
    const int2* stage_tab;        // staging table (snet_layout), entries ordered by layer
    int stage_n;                  // all entries (forward)
    int stage_bwd0;               // first entry of layer 1: the backward kernel stages [stage_bwd0, stage_n)
    int lh[DCV_MAX_LAYERS + 1];   // LDS float offset of H_l [TR][ps_l]   (H_0 = the input tile)
    int ps[DCV_MAX_LAYERS + 1];
    int act_len;                  // floats of the activation region [lh[0], lh[0] + act_len): the blob of a workgroup
    const float* params;
    const float* img;             // global weight image in the LDS layout (snet.hip: snet_image_build), or null: table-driven staging
    int img_floats;               //   floats of the whole image; the backward stages [img_bwd0, img_floats): layers >= 1
    int img_bwd0;
    const float* Xn;
    int64_t ld;
    RowMap rows;                  // half = batch: logical row p < B is x_t of pair p, row B + p its x_lag
    int B;                        // pairs of this rank's batch
    int nb, wgpb;                 // batches of this launch (> 1: evaluation with the fused head only) and workgroups per batch
    int d;                        // network outputs (<= 4)
    int store_blob;
    float* blob;                  // [workgroups][blob_stride]
    int64_t blob_stride;
    double* spart;                // statistics partials [workgroups][2d + 2d^2]
    unsigned* ticket;
    double* stats;
    FusedHead fused;
    const double* gradp;          // backward: [mu d | Gu d*d | Gv d*d | c d]
    float* part;                  // backward: gradient partials
};

union TicaWaveLdsAny {
    TicaWaveLds<1> h1;
    TicaWaveLds<2> h2;
    TicaWaveLds<3> h3;
    TicaWaveLds<4> h4;
};
// the wave-parallel d x d loss head (loss_head.h) for the run-time d of the plan
__device__ __forceinline__ void snet_dt_head(int D, TicaWaveLdsAny& w, const double* stats, const FusedHead& f, double* gradp, double* log,
                                             int* log_count, int log_cap, int lane) {
    switch (D) {
        case 1: tica_grad_wave<1>(w.h1, stats, f.Bg, f.reg, gradp, log, log_count, log_cap, f.log_width, lane); break;
        case 2: tica_grad_wave<2>(w.h2, stats, f.Bg, f.reg, gradp, log, log_count, log_cap, f.log_width, lane); break;
        case 3: tica_grad_wave<3>(w.h3, stats, f.Bg, f.reg, gradp, log, log_count, log_cap, f.log_width, lane); break;
        default: tica_grad_wave<4>(w.h4, stats, f.Bg, f.reg, gradp, log, log_count, log_cap, f.log_width, lane); break;
    }
}
// TR rows per workgroup = TR / 2 pairs (16 for small batches, 32, 64 or 128: larger tiles mean fewer statistics / gradient partials for the
// ticketed sums and the reduction launch behind; the work of a tile is latency, not arithmetic, at these widths)
template <int TR>
__global__ __launch_bounds__(kSnetThreads) void snet_dt_fwd_kernel(SnetDtArgs a) {
    constexpr int NT = kSnetThreads, HP = TR / 2;
    constexpr int XU = TR / 8;   // 16-byte units of the input tile per thread (TR * pin / 4 <= XU * NT: pin <= 256 * 32 / TR ... checked by the plan)
    const int D = a.d, W = 2 * D + 2 * D * D;
    extern __shared__ __attribute__((aligned(16))) float sl[];
    __shared__ TicaWaveLdsAny s_head;
    __shared__ double s_stat[40];
    __shared__ unsigned s_flag;
    __shared__ int s_slot;
    const SnetCoords<TR> k;
    const int t = k.t, lane = k.lane, wave = k.wave;
    const int L = a.L;
    const unsigned ka_touch = snet_touch_kernargs<(int)sizeof(SnetDtArgs)>();
    // ---- input tile: local row r is pair p0 + r % HP, half r / HP
    // workgroup -> (batch of the launch, tile of the batch); batch j of a batched evaluation = the pairs [j * B, (j + 1) * B)
    const int bj = a.nb > 1 ? (int)blockIdx.x / a.wgpb : 0;
    const unsigned wgpb = a.nb > 1 ? (unsigned)a.wgpb : gridDim.x, wg0 = (unsigned)bj * wgpb;
    const int64_t p0 = (int64_t)(blockIdx.x - wg0) * HP;
    RowMap rows = a.rows;
    if (bj != 0) {
        if (rows.idx != nullptr) rows.idx += (int64_t)bj * a.B;
        rows.row0 += (int64_t)bj * a.B;
    }
    const int F0 = a.l[0].in, pin0 = a.l[0].pin, ps0 = a.ps[0];
    float* H0 = sl + a.lh[0];
    const bool x_vec = (F0 & 3) == 0 && (a.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Xn) & 15) == 0;
    const int x_sh = a.l[0].c4_shift, x_tot = TR << x_sh;
    auto src_row = [&](int r) -> int64_t {   // matrix row of local row r, -1 past the batch
        const int half = r >= HP ? 1 : 0;
        const int64_t p = p0 + (r - half * HP);
        return p < a.B ? rows.template get<true>(half ? (int64_t)a.B + p : p) : -1;
    };
    constexpr int XA = XU < 8 ? XU : 8;   // units that ride along the weight staging; the rest (TR = 128) in a second batch
    float4 xv[XA];
    bool x_issued = false;
    auto load_x = [&](int u) -> float4 {
        const int f4 = F0 >> 2;
        const int i = t + NT * u, r = i >> x_sh, c = i - (r << x_sh);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < x_tot && c < f4) {
            const int64_t row = src_row(r);
            if (row >= 0) v = *reinterpret_cast<const float4*>(a.Xn + row * a.ld + 4 * c);
        }
        return v;
    };
    auto store_x = [&](int u, const float4& v) {
        const int i = t + NT * u, r = i >> x_sh, c = i - (r << x_sh);
        if (i < x_tot) *reinterpret_cast<float4*>(H0 + r * ps0 + 4 * c) = v;
    };
    auto issue_x = [&]() {
        if (!x_vec || x_issued) return;
        x_issued = true;
#pragma unroll
        for (int u = 0; u < XA; ++u) xv[u] = load_x(u);
    };
    // ---- stage every weight image and bias
    if (a.img != nullptr) {   // one contiguous LDS-DMA copy of the weight image (kept current by the optimiser), the input rows behind it
        snet_stage_image<NT>(a.img, sl, 0, a.img_floats, t);
    } else {   // through the plan's staging table, the rows of X riding along the first pass's data round trip
        snet_stage_table<NT, false>(a.stage_tab, 0, a.stage_n, a.params, sl, t, issue_x);
    }
    issue_x();
    if (a.img != nullptr) vm_wait<0>();   // this wave's image copies have landed (the barrier below covers the other waves)
    asm volatile("" ::"s"(ka_touch));
    if (x_vec) {
#pragma unroll
        for (int u = 0; u < XA; ++u) store_x(u, xv[u]);
        if constexpr (XU > XA) {
            float4 xw[XU - XA];
#pragma unroll
            for (int u = XA; u < XU; ++u) xw[u - XA] = load_x(u);
#pragma unroll
            for (int u = XA; u < XU; ++u) store_x(u, xw[u - XA]);
        }
    } else {
        for (int i = t; i < TR * pin0; i += NT) {
            const int r = i / pin0, c = i - r * pin0;
            float v = 0.f;
            if (c < F0) {
                const int64_t row = src_row(r);
                if (row >= 0) v = a.Xn[row * a.ld + c];
            }
            H0[r * ps0 + c] = v;
        }
    }
    __syncthreads();
    // ---- forward chain
    for (int l = 0; l < L; ++l) {
        const SnetLayer& y = a.l[l];
        const float* Hin = sl + a.lh[l];
        float* Hout = sl + a.lh[l + 1];
        const int psin = a.ps[l], pso = a.ps[l + 1];
        snet_forward_layer<TR>(k, y, sl, Hin, psin, Hout, pso, [](sv4f&, int) {});
        __syncthreads();
    }
    // ---- statistics partial of the tile's pairs: [sum f_t | sum f_lag | sum f_t f_t^T | sum f_t f_lag^T], float64, pair order
    {
        const float* FL = sl + a.lh[L];
        const int psL = a.ps[L];
        const int64_t left = (int64_t)a.B - p0;
        const int nvalid = left >= HP ? HP : (left > 0 ? (int)left : 0);
        if (t < W) {
            const double s = tica_stat_entry(t, D, nvalid, [&](int pl, int i) { return (double)FL[pl * psL + i]; },
                                             [&](int pl, int i) { return (double)FL[(HP + pl) * psL + i]; });
            handoff_store(a.spart + (int64_t)blockIdx.x * W + t, s);
        }
    }
    // ---- the tile's activations (input tile, every layer's output) for the backward launch: one contiguous blob
    if (a.store_blob) {
        const float* src = sl + a.lh[0];
        float* dst = a.blob + (int64_t)blockIdx.x * a.blob_stride;
        for (int i = 4 * t; i < a.act_len; i += 4 * NT) {
            const sv4f v = *reinterpret_cast<const sv4f*>(src + i);
            handoff_store16(dst + i, v);   // write-through: nothing left for the write-back at the end of the launch
        }
    }
    // ---- last workgroup: the partials in block order, then the d x d loss head
    if (!handoff_arrive_last(a.ticket + bj, wgpb, &s_flag)) return;
    {
        // (the group sums go where the weight images were: they are dead)
        const double s = block_sum_partials_in_order(a.spart + (int64_t)wg0 * W, wgpb, W, NT / W, t, reinterpret_cast<double*>(sl));
        if (t < W) {
            if (a.nb <= 1) a.stats[t] = s;
            s_stat[t] = s;
        }
        if (a.fused.on) {
            __syncthreads();
            if (wave == 0) {
                const FusedHead& f = a.fused;
                // a batched evaluation appends its records in batch order (loss_head.h: log_member): the head of batch j moves a
                // private copy of the counter, the last head to finish moves the counter itself by nb
                MemberLog ml{f.log, f.log_cap};
                int* lc = f.log_count;
                int slot0 = 0;
                if (a.nb > 1) {
                    slot0 = *f.log_count;
                    asm volatile("s_waitcnt vmcnt(0) ; the counter has been read" ::: "memory");
                    if (lane == 0) s_slot = slot0;
                    wave_sync_lds();
                    ml = log_member(f.log, f.log_width, f.log_cap, bj);
                    lc = &s_slot;
                }
                snet_dt_head(D, s_head, s_stat, f, f.gradp, ml.log, lc, ml.cap, lane);
                if (a.nb > 1 && lane == 0) log_advance_by_ticket(a.ticket + a.nb, a.nb, f.log_count, slot0);
            }
        }
    }
}

template <int TR>
__global__ __launch_bounds__(kSnetThreads) void snet_dt_bwd_kernel(SnetDtArgs a) {
    constexpr int NT = kSnetThreads, HP = TR / 2;
    const int D = a.d, NG = 2 * D + 2 * D * D;   // mu | Gu | Gv | c
    extern __shared__ __attribute__((aligned(16))) float sl[];
    __shared__ double s_g[40];
    __shared__ double s_stat[40];
    __shared__ TicaWaveLdsAny s_head;
    const SnetCoords<TR> k;
    const int t = k.t, lane = k.lane, wave = k.wave;
    const int L = a.L;
    const unsigned ka_touch = snet_touch_kernargs<(int)sizeof(SnetDtArgs)>();
    const int64_t p0 = (int64_t)blockIdx.x * HP;
    // ---- stage the weight images of layers >= 1 (the input gradients read them; no bias, no layer 0) and the blob.
    //      Order of issue: table entries, the first eight blob units, the weight data (needs the entries: loads return in
    //      order, so waiting for the entries does not wait for the blob), LDS stores at the end.
    const float* bsrc = a.blob + (int64_t)blockIdx.x * a.blob_stride;
    float* bdst = sl + a.lh[0];
    const int n4 = a.act_len >> 2;
    float4 bv[8];
    bool blob_issued = false;
    auto issue_blob = [&]() {
        if (blob_issued) return;
        blob_issued = true;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = t + NT * u;
            bv[u] = i < n4 ? *reinterpret_cast<const float4*>(bsrc + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // The d x d loss head HERE, by the last wave of every workgroup, from the batch statistics the forward launch left
    // (all-reduced in between in a data-parallel step): ~3 us of dependent float64 algebra that sat on the forward launch's
    // critical path (its last arriver, the whole chip waiting) now runs while this wave's staging loads are in flight and
    // the other waves stage theirs.  Every workgroup computes the same matrices (deterministic: same inputs, same code);
    // the first one appends the loss record.
    auto run_head = [&]() {
        if (!a.fused.on) return;
        if (wave == kSnetWaves - 1) {
            if (lane < NG) s_stat[lane] = a.stats[lane];
            wave_sync_lds();
            const FusedHead& f = a.fused;
            double* logp = blockIdx.x == 0 ? f.log : nullptr;
            int* lc = blockIdx.x == 0 ? f.log_count : nullptr;
            snet_dt_head(D, s_head, s_stat, f, s_g, logp, lc, f.log_cap, lane);
        }
    };
    if (a.img != nullptr) {   // layers >= 1 of the weight image by LDS-DMA, the blob's first units behind it
        snet_stage_image<NT>(a.img, sl, a.img_bwd0, a.img_floats, t);
    } else {   // through the plan's staging table from layer 1 on, the blob's first units ahead of the first pass's data loads
        snet_stage_table<NT, true>(a.stage_tab, a.stage_bwd0, a.stage_n, a.params, sl, t, issue_blob);
    }
    issue_blob();
    // After the staging loop on both paths: the head is wave-wide (its lanes share data through LDS) and must run with the
    // whole wave.  Inside the table loop only the lanes with an entry left take the last pass, so a staging table of
    // 449..511 entries in the backward ran it twice under partial exec masks, each time with part of the statistics.
    run_head();
    if (a.img != nullptr) vm_wait<0>();   // (the blob loads above are covered too)
    if (!a.fused.on && t < NG) s_g[t] = a.gradp[t];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int i = t + NT * u;
        if (i < n4) *reinterpret_cast<float4*>(bdst + 4 * i) = bv[u];
    }
    for (int i0 = t + 8 * NT; i0 < n4; i0 += 8 * NT) {   // larger tiles: the rest of the blob, eight units in flight
        float4 w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + NT * u;
            w[u] = i < n4 ? *reinterpret_cast<const float4*>(bsrc + 4 * i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + NT * u;
            if (i < n4) *reinterpret_cast<float4*>(bdst + 4 * i) = w[u];
        }
    }
    asm volatile("" ::"s"(ka_touch));
    __syncthreads();
    // ---- loss gradient of the tile's pairs, float64, rounded once (loss_head.h: tica_grad_t / tica_grad_l; the rows of the
    //      exact gradient sum to zero over the batch, see DESIGN.md section 2, noise-driven parameters); times act'(f) of the
    //      last layer; written over f (H_L becomes dZ_L)
    {
        float* FL = sl + a.lh[L];
        const int psL = a.ps[L];
        const int act_last = a.l[L - 1].act;
        const int pl = t / D, i = t - pl * D;
        const bool mine = t < HP * D;
        const bool valid = mine && p0 + pl < a.B;
        float ft[4], fg[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ft[k] = (mine && k < D) ? FL[pl * psL + k] : 0.f;
            fg[k] = (mine && k < D) ? FL[(HP + pl) * psL + k] : 0.f;
        }
        __syncthreads();   // every thread has read its pair before any value is overwritten
        if (mine) {
            float gt = 0.f, gl = 0.f;
            if (valid) {
                // the two chains of loss_head.h (tica_grad_t, tica_grad_l) side by side, sharing u and the loads of Gv: composed from
                // the two functions the kernel was 43 instructions longer and measured slower (profiles/loss_head_resource_usage.md)
                const double* mu = s_g;
                const double* Gu = s_g + D;
                const double* Gv = Gu + D * D;
                const double* cv = Gv + D * D;
                double g1 = cv[i], g2 = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < D) {
                        const double u = (double)ft[k] - mu[k], v = (double)fg[k] - mu[k];
                        g1 = fma(Gu[i * D + k], u, g1);
                        g1 = fma(Gv[i * D + k], v, g1);
                        g2 = fma(Gv[i * D + k], u, g2);
                    }
                }
                float fti = ft[0], fgi = fg[0];   // ft[i] / fg[i] without a dynamically indexed register array
#pragma unroll
                for (int k = 1; k < 4; ++k) {
                    fti = i == k ? ft[k] : fti;
                    fgi = i == k ? fg[k] : fgi;
                }
                gt = (float)g1 * act_grad_from_out(act_last, fti);
                gl = (float)g2 * act_grad_from_out(act_last, fgi);
            }
            FL[pl * psL + i] = gt;
            FL[(HP + pl) * psL + i] = gl;
        }
        __syncthreads();
    }
    // ---- backward chain (snet_ae_kernel): dZ_l lives in the buffer of H_{l+1}; dZ_{l-1} is written over H_l once the weight
    //      gradient of layer l (which reads H_l) has been formed by every wave
    for (int l = L - 1; l >= 0; --l) {
        const SnetLayer& y = a.l[l];
        const float* dZ = sl + a.lh[l + 1];
        float* Hin = sl + a.lh[l];
        const int psz = a.ps[l + 1], psh = a.ps[l];
        sv4f dg[kSnetMaxTiles];
        if (l > 0) snet_dgrad_layer<TR>(k, y, sl, dZ, psz, dg);   // input gradient first, kept in registers
        snet_wgrad_partials<TR>(k, y, a.part, Hin, psh, dZ, psz);
        snet_bgrad_partials<TR>(k, y, a.part, dZ, psz);
        if (l == 0) break;
        __syncthreads();   // every wave is done reading H_l
        const int act_prev = a.l[l - 1].act, out_prev = a.l[l - 1].out;
        snet_dz_prev<TR>(k, y, act_prev, out_prev, Hin, psh, dg);
        __syncthreads();
    }
}

struct SnetDtPlan {
    SnetDtArgs base;       // layer table, staging table; the activation map is laid out per launch (it depends on TR)
    int fl;                // LDS floats of the weight images
    int64_t per_wg;        // floats of one workgroup's gradient partials (dense)
    int2* stage_tab;
    float* part;           // gradient partials
    int64_t part_floats;
    float* blob;
    int64_t blob_floats;
    double* spart;         // statistics partials
    int64_t spart_n;
    unsigned* ev_ticket;   // batched evaluation: one ticket per batch + the one that moves the log counter (zero between launches)
    int64_t ev_ticket_n;
    int64_t last_wg;       // workgroups and tile rows of the last forward (the backward launches the same grid)
    int last_tr;
};
constexpr size_t kSnetDtLdsMax = 160 * 1024 - 8 * 1024;   // static LDS of the kernels (loss head, flags) and a margin

// activation map of a TR-row tile behind the weight images; returns the LDS floats needed
static int snet_dt_map(SnetDtArgs& a, int fl, int TR) {
    const int f = snet_act_map(a.l, a.L, TR, fl, a.lh, a.ps);
    a.act_len = f - a.lh[0];
    return f < 2048 ? 2048 : f;   // the last arriver sums the statistics partials in the first 4 KB
}
// rows per tile for a batch of B pairs: the smallest tile that keeps the launch at <= 256 workgroups (one per CU; the ticketed
// partial sums and the gradient reduction walk one partial per workgroup), provided the tile fits: TR * pin / 4 <= (TR / 8) * 512
// input units per thread (pin <= 64 * 32 / TR ... i.e. always for pin <= 256 at TR = 32, pin <= 256 at 64 and 128 too since
// the unit count per thread grows with TR) and the activation map fits in LDS
static int snet_dt_pick_tr(const SnetDtPlan* pl, int64_t B) {
    static const int tr_env = (int)env_int("DCV_SNET_TR", 0);
    int best = 0;
    // 16-row tiles (8 pairs per workgroup) up to 1024 pairs: a shorter latency chain per workgroup while the twice-as-many
    // partials stay cheap.  A/B on one box, 54-16-8-2, contiguous batches (tools/dbg/dt_tr_probe.py): 24.2 -> 23.2 us per step
    // at 64 pairs, 24.7 -> 23.7 at 128, 25.5 -> 23.9 at 256, 25.4 -> 24.6 at 512, 26.1 -> 24.7 at 1024, and 26.1 -> 26.8
    // (slower) at 2048; the gathered batch of 128 of bench.py's ref_small block: 29.1 -> 27.2.  DCV_SNET_DT16=0 turns them off.
    static const bool dt16 = env_not("DCV_SNET_DT16", '0');
    // (128-64-32-4 on the same box, 16 | 32 rows: 25.8 | 28.0 at 128 pairs, 27.9 | 29.3 at 1024 -- 5.4 MB of partials and still ahead --
    // 32.4 | 30.4 at 2048, 53 | 35 at 4096: two rounds of the chip)
    if (tr_env == 16 || (tr_env == 0 && dt16 && cdiv(B, 8) <= 128)) {
        SnetDtArgs tmp = pl->base;
        if ((size_t)snet_dt_map(tmp, pl->fl, 16) * sizeof(float) <= kSnetDtLdsMax) return 16;
    }
    for (int TR : {32, 64, 128}) {
        SnetDtArgs tmp = pl->base;
        if ((size_t)snet_dt_map(tmp, pl->fl, TR) * sizeof(float) > kSnetDtLdsMax) break;
        // the backward keeps a layer's input-gradient tiles of a wave in registers: kSnetMaxTiles * (8 waves / (TR / 16) row groups)
        // column tiles of 16 must cover the widest hidden layer
        bool fits = true;
        for (int l = 1; l < tmp.L; ++l) fits = fits && tmp.l[l].nk_in <= kSnetMaxTiles * (kSnetWaves / (TR / 16));
        if (!fits) break;
        if (tr_env != 0) {
            if (tr_env == TR) return TR;
            continue;
        }
        best = TR;
        if (cdiv(B, TR / 2) <= 256) break;   // one round of the chip; measured at 4096 pairs: 128 tiles of 64 rows 41.8 us / step, 256 of 32 rows 38.2
    }
    return best;
}

static bool snet_dt_build(dcv_mlp* m) {
    if (m->desc.model != DCV_MODEL_DEEPTICA || m->any_drop || m->any_bn || m->d_out > 4 || m->d_out < 1 || snet_disabled()) return false;
    SnetDtPlan* pl = new (std::nothrow) SnetDtPlan();   // value-initialised: no buffer yet
    if (!pl) return false;
    m->snet_dt = pl;   // from here on a half-built plan is released by snet_dt_free
    auto fail = [&] {
        snet_dt_free(m);
        return false;
    };
    SnetDtArgs& a = pl->base;
    a.L = m->L;
    a.d = m->d_out;
    std::vector<int2> tab;
    int tab_begin[DCV_MAX_LAYERS];
    if (!snet_layout(m, a.l, tab, tab_begin, pl->fl, pl->per_wg)) return fail();
    (void)snet_image_build(m);   // on failure the kernels keep the table-driven staging
    {
        SnetDtArgs tmp = a;
        if ((size_t)snet_dt_map(tmp, pl->fl, 32) * sizeof(float) > kSnetDtLdsMax) return fail();
    }
    if (!snet_upload_table(tab, &pl->stage_tab)) return fail();
    a.stage_tab = pl->stage_tab;
    a.stage_n = (int)tab.size();
    a.stage_bwd0 = m->L > 1 ? tab_begin[1] : (int)tab.size();
    // batched validation passes: statistics partials and tickets for the bounds of dcv_mlp_eval_steps, allocated now so that no
    // allocation lands in a timed pass (without them the passes go batch by batch)
    if (snet_grow(&pl->spart, &pl->spart_n, kEvalWorkgroupsPerLaunch * (int64_t)m->stats_len) && snet_grow(&pl->ev_ticket, &pl->ev_ticket_n, (int64_t)kEvalBatchesPerLaunch + 1)) {
        if (hipMemset(pl->ev_ticket, 0, (size_t)pl->ev_ticket_n * sizeof(unsigned)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(pl->ev_ticket);
            pl->ev_ticket = nullptr;
            pl->ev_ticket_n = 0;
        }
    }
    // as in snet_build: the null-stream memset above must have landed before the first step launches on the caller's stream
    if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return fail();
    }
    return true;
}

void snet_dt_free(dcv_mlp* m) {
    SnetDtPlan* pl = static_cast<SnetDtPlan*>(m->snet_dt);
    if (!pl) return;
    if (pl->part) (void)hipFree(pl->part);
    if (pl->blob) (void)hipFree(pl->blob);
    if (pl->spart) (void)hipFree(pl->spart);
    if (pl->ev_ticket) (void)hipFree(pl->ev_ticket);
    if (pl->stage_tab) (void)hipFree(pl->stage_tab);
    delete pl;
    m->snet_dt = nullptr;
}

int snet_dt_last_tile_rows(const dcv_mlp* m) {
    const SnetDtPlan* pl = static_cast<const SnetDtPlan*>(m->snet_dt);
    return pl ? pl->last_tr : 0;
}

static int g_dt_attr_state[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per kernel instantiation (snet_launch): forward TR 32 / 64 / 128 / 16, then the backward's
template <class K>
static int snet_dt_launch(K kern, int slot, size_t lds_bytes, const SnetDtArgs& a, int64_t nwg, hipStream_t s) {
    return snet_launch(kern, g_dt_attr_state[slot], kSnetDtLdsMax, lds_bytes, a, nwg, s);
}

// Fused forward of one Deep-TICA batch (+ batch statistics, + the loss head when head != 0: 1 = training, the head's
// matrices go to m->gradp; 2 = evaluation).  keep_blob: a backward may follow.  Returns 1 when the fused form does not
// apply (the caller runs the layer-by-layer path), DCV_OK when the launch was enqueued.
// nb > 1 (head == 2, no blob): nb batches of `batch` pairs each in the one launch, one loss record per batch in batch order.
int snet_dt_forward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int head, bool keep_blob,
                    hipStream_t s, int nb) {
    static const int64_t kMaxBytes = 64ll << 20;
    if (!snet_plan_ready(m->snet_dt, m->snet_dt_tried, [&] { return snet_dt_build(m); })) return 1;
    SnetDtPlan* pl = static_cast<SnetDtPlan*>(m->snet_dt);
    const int TR = snet_dt_pick_tr(pl, batch);
    if (TR == 0) return 1;
    SnetDtArgs a = pl->base;
    const size_t lds_bytes = (size_t)snet_dt_map(a, pl->fl, TR) * sizeof(float);
    const int64_t wgpb = cdiv(batch, TR / 2);
    const int W = m->stats_len;
    if (wgpb > 512 || wgpb * pl->per_wg * (int64_t)sizeof(float) > kMaxBytes || wgpb * a.act_len * (int64_t)sizeof(float) > kMaxBytes) return 1;
    if (nb < 1 || (nb > 1 && (head != 2 || keep_blob))) return 1;
    const int64_t nwg = wgpb * nb;
    if (!snet_grow(&pl->spart, &pl->spart_n, nwg * W)) return 1;
    if (nb > 1 && nb + 1 > pl->ev_ticket_n) return 1;   // (sized by snet_dt_build for the bounds of dcv_mlp_eval_steps)
    if (keep_blob && !snet_grow(&pl->blob, &pl->blob_floats, nwg * (int64_t)a.act_len)) return 1;
    a.params = m->params;
    a.img = m->snet_img;
    a.img_floats = m->snet_img_floats;
    a.img_bwd0 = m->L > 1 ? a.l[1].lw : m->snet_img_floats;
    a.Xn = Xn_d;
    a.ld = ld;
    a.rows = RowMap{idx_d, row0, batch, m->desc.lag};
    a.B = batch;
    a.nb = nb;
    a.wgpb = (int)wgpb;
    a.store_blob = keep_blob && pl->blob != nullptr ? 1 : 0;
    a.blob = pl->blob;
    a.blob_stride = a.act_len;
    a.spart = pl->spart;
    a.ticket = nb > 1 ? pl->ev_ticket : m->ticket;
    a.stats = m->stats;
    a.fused = FusedHead{0, 0.0, 0.0, nullptr, nullptr, nullptr, 0, 0};
    if (head) a.fused = FusedHead{1, (double)batch, m->desc.tica_reg, head == 1 ? m->gradp : nullptr, m->log, m->log_count, m->log_cap, m->log_width};
    a.gradp = nullptr;
    a.part = nullptr;
    pl->last_wg = nb > 1 ? -1 : nwg;   // (no backward behind a batched evaluation)
    pl->last_tr = TR;
    switch (TR) {
        case 16: return snet_dt_launch(snet_dt_fwd_kernel<16>, 3, lds_bytes, a, nwg, s);
        case 32: return snet_dt_launch(snet_dt_fwd_kernel<32>, 0, lds_bytes, a, nwg, s);
        case 64: return snet_dt_launch(snet_dt_fwd_kernel<64>, 1, lds_bytes, a, nwg, s);
        default: return snet_dt_launch(snet_dt_fwd_kernel<128>, 2, lds_bytes, a, nwg, s);
    }
}

// Fused backward of the batch whose forward snet_dt_forward ran last (its blob is in place): gradient partials for the
// reduction, whose descriptors go to `ra`.  head: the loss head has not run yet -- every workgroup evaluates it from m->stats
// (the sums over the GLOBAL batch) and the first one appends the loss record; otherwise m->gradp holds the head's matrices.
int snet_dt_backward(dcv_mlp* m, int32_t batch, int64_t global_batch, bool head, ReduceArgsView* ra, hipStream_t s) {
    SnetDtPlan* pl = static_cast<SnetDtPlan*>(m->snet_dt);
    if (!pl || !pl->blob) {
        set_error("snet_dt_backward: no fused forward to go back through");
        return DCV_ESTATE;
    }
    const int TR = pl->last_tr;
    const int64_t nwg = cdiv(batch, TR / 2);
    if (nwg != pl->last_wg) {
        set_error("snet_dt_backward: batch=%d does not match the fused forward", batch);
        return DCV_ESTATE;
    }
    const int64_t part_need = nwg * pl->per_wg + 8 * (int64_t)m->L;
    if (!snet_grow(&pl->part, &pl->part_floats, part_need)) {
        set_error("snet_dt_backward: out of device memory (%lld floats of gradient partials)", (long long)part_need);
        return DCV_ENOMEM;
    }
    SnetDtArgs a = pl->base;
    const size_t lds_bytes = (size_t)snet_dt_map(a, pl->fl, TR) * sizeof(float);
    snet_partials_layout(a.l, m->L, nwg, pl->part, ra);
    a.params = m->params;
    a.img = m->snet_img;
    a.img_floats = m->snet_img_floats;
    a.img_bwd0 = m->L > 1 ? a.l[1].lw : m->snet_img_floats;
    a.B = batch;
    a.blob = pl->blob;
    a.blob_stride = a.act_len;
    a.gradp = m->gradp;
    a.part = pl->part;
    a.stats = m->stats;
    a.fused = FusedHead{0, 0.0, 0.0, nullptr, nullptr, nullptr, 0, 0};
    if (head) a.fused = FusedHead{1, (double)global_batch, m->desc.tica_reg, nullptr, m->log, m->log_count, m->log_cap, m->log_width};
    switch (TR) {
        case 16: return snet_dt_launch(snet_dt_bwd_kernel<16>, 7, lds_bytes, a, nwg, s);
        case 32: return snet_dt_launch(snet_dt_bwd_kernel<32>, 4, lds_bytes, a, nwg, s);
        case 64: return snet_dt_launch(snet_dt_bwd_kernel<64>, 5, lds_bytes, a, nwg, s);
        default: return snet_dt_launch(snet_dt_bwd_kernel<128>, 6, lds_bytes, a, nwg, s);
    }
}

}  // namespace dcv

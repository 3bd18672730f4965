// Fused training / evaluation step of a SMALL network: every weight of the MLP resident in one CU's LDS.
//
// The reference's own configurations are small networks (its autoencoder test model is 54-16-8-2-4-8-54; BASELINE C2 is
// 128-64-32-2-32-64-128 = 82 KB of parameters).  Layer by layer, such a step is ~20 launches of 5-16 us each on a
// few thousand rows -- launch- and latency-bound, < 2 % of any roofline.  Here ONE launch does the whole step for the
// autoencoder: a workgroup stages all weights into LDS once (padded rows: conflict-free 128-bit fragment reads), takes a
// tile of TR rows, runs the forward chain with the activations kept in LDS, forms the loss gradient in the epilogue of
// the last layer, and walks back through the layers -- weight gradient of the tile (contraction over its TR rows) and
// input gradient, the latter written over the activation it consumes -- without an activation ever leaving the CU.
// Out: one gradient partial per workgroup and layer (slab layout of the split-K reduction, so reduce_grads_small_kernel
// + the fused optimiser update finish the step), the squared-error partial, and through a ticketed hand-off (handoff.h)
// the step's loss record.
//
// Arithmetic: v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulate) in both arithmetic flavours of the library --
// the network is far too small for the matrix rate to matter, and no operand splitting is needed.
// A wave owns 16-row groups: TR = 32 -> waves (row group, column-tile parity); the k-slot permutation of gemm.h lets
// one ds_read_b128 feed four MFMA steps (lane (n, q) holds k = k0 + 4q + s in step s, identically for A and B).
#include "snet.h"
#include "loss_head.h"
#include <new>

namespace dcv {

struct SnetArgs {
    SnetLayer l[DCV_MAX_LAYERS];
    int L;
    const int2* stage_tab;        // staging table: per 16-byte unit of the LDS image {source element offset into params or -1,
                                  // LDS float offset | valid elements << 20 | 16-byte load legal << 24}
    int stage_n;
    int lh[DCV_MAX_LAYERS + 1];   // LDS float offset of H_l [TR][ps_l]   (H_0 = the input tile)
    int ps[DCV_MAX_LAYERS + 1];   // row stride of H_l = padded width + 4
    int lred;                     // LDS float offset of the reduction scratch (kSnetThreads doubles)
    const float* params;
    const float* img;             // global weight image in the LDS layout (snet_image_build), or null: table-driven staging
    int img_floats;
    const float* Xn;
    int64_t ld;
    RowMap rows;
    int64_t R;                    // rows of one batch
    int nb, wgpb;                 // batches of this launch (> 1: evaluation only, snet_ae_eval_batches) and workgroups per batch
    const float* range;
    float scale;                  // 2 / (global batch * F)
    int train;
    float* part;
    double* sse_part;
    unsigned* ticket;
    double* stats;
    double Bg;
    double* log;
    int* log_count;
    int log_cap, log_width;
    // variational autoencoder (DCV_MODEL_VAE): Linear vae_l (the first decoder Linear) reads z = mu + exp(lv / 2) * eps, sampled
    // from the heads' output H_{vae_l} = [mu | lv] into its own tile Z [TR][pz]; vae_l = -1 for the autoencoder
    int vae_l, vae_d;
    int lz, pz;
    const float* eps;             // eps rows of the launch's first batch (batch j: + j * R * vae_d), dense [rows][vae_d]
    double beta;                  // weight of the KL term
    float beta_b;                 // beta / global batch
    double* kl_part;              // per-workgroup KL partials (beside sse_part, through the same hand-off)
    unsigned long long* stamps;   // diagnostic (dcv_debug_snet_stamps): s_memrealtime of workgroup 0 at the phase boundaries, or null
};
#define SNET_STAMP(k)                                                                          \
    do {                                                                                        \
        if (a.stamps != nullptr && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[k] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

// VAE: the variational autoencoder's form (z sampling, KL partials, dL/dz -> [dL/dmu | dL/dlv]); a separate instantiation, so the
// autoencoder's kernel keeps its register budget
template <int TR, bool VAE>
__global__ __launch_bounds__(kSnetThreads) void snet_ae_kernel(SnetArgs a) {
    constexpr int NT = kSnetThreads;
    extern __shared__ __attribute__((aligned(16))) float sl[];
    const SnetCoords<TR> k;
    const int t = k.t, lane = k.lane, wave = k.wave;
    const int L = a.L;
    const unsigned ka_touch = snet_touch_kernargs<(int)sizeof(SnetArgs)>();
    SNET_STAMP(0);
    // ---- input tile H_0 (rows past the batch: zeros): with 16-byte loads the whole tile is at most four units per thread
    //      (TR * pin / 4 <= 4 * NT); they are issued inside the weight staging, behind its data loads, and written to LDS
    //      after it
    // workgroup -> (batch of the launch, tile of the batch): one batch unless this is a batched evaluation (nb > 1), whose
    // batch j covers the logical rows [j * R, (j + 1) * R) of the row map
    const int bj = a.nb > 1 ? (int)blockIdx.x / a.wgpb : 0;
    const int tile0 = (int)blockIdx.x - bj * a.wgpb;
    const int64_t r0 = (int64_t)tile0 * TR;
    RowMap rows = a.rows;
    if (bj != 0) {
        if (rows.idx != nullptr) rows.idx += (int64_t)bj * a.R;
        rows.row0 += (int64_t)bj * a.R;
    }
    const int F0 = a.l[0].in, p0 = a.l[0].pin, ps0 = a.ps[0];
    float* H0 = sl + a.lh[0];
    const bool x_vec = (F0 & 3) == 0 && (a.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Xn) & 15) == 0;
    const int x_sh = a.l[0].c4_shift, x_tot = TR << x_sh;
    float4 xv[4];
    bool x_issued = false;
    auto issue_x = [&]() {
        if (!x_vec || x_issued) return;
        x_issued = true;
        const int f4 = F0 >> 2;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = t + NT * u, r = i >> x_sh, c = i - (r << x_sh);
            xv[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < x_tot && r0 + r < a.R && c < f4) xv[u] = *reinterpret_cast<const float4*>(a.Xn + rows.template get<true>(r0 + r) * a.ld + 4 * c);
        }
    };
    // ---- stage every weight image and bias (zero-padded, row stride pin + 4)
    if (a.img != nullptr) {
        // one contiguous LDS-DMA copy of the whole weight image (kept current by the optimiser: OptArgs::img); the input rows
        // are requested right behind it
        snet_stage_image<NT>(a.img, sl, 0, a.img_floats, t);
    } else {
        // through the plan's staging table, the input rows behind the first pass's data loads
        snet_stage_table<NT, false>(a.stage_tab, 0, a.stage_n, a.params, sl, t, issue_x);
    }
    issue_x();   // (behind the image copy; after the table: a plan without staging units, not reachable, kept for the invariant xv is loaded)
    asm volatile("" ::"s"(ka_touch));   // the touches have landed
    if (a.img != nullptr) vm_wait<0>();   // the image copies of this wave have landed (the barrier below covers the other waves)
    SNET_STAMP(1);
    if (x_vec) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = t + NT * u, r = i >> x_sh, c = i - (r << x_sh);
            if (i < x_tot) *reinterpret_cast<float4*>(H0 + r * ps0 + 4 * c) = xv[u];
        }
    } else {
        for (int i = t; i < TR * p0; i += NT) {
            const int r = i / p0, c = i - r * p0;
            float v = 0.f;
            if (r0 + r < a.R && c < F0) v = a.Xn[rows.template get<true>(r0 + r) * a.ld + c];
            H0[r * ps0 + c] = v;
        }
    }
    __syncthreads();
    SNET_STAMP(2);
    // ---- forward chain
    double sse = 0.0, kl = 0.0;
    for (int l = 0; l < L; ++l) {
        const SnetLayer& y = a.l[l];
        if (VAE && l == a.vae_l) {
            // VAE: z = eps * exp(lv / 2) + mu into the Z tile (zero padding and rows past the batch), KL terms of the tile's rows
            const int d = a.vae_d, psh = a.ps[l];
            const float* Hh = sl + a.lh[l];
            float* Z = sl + a.lz;
            const float* ep = a.eps + ((int64_t)bj * a.R + r0) * d;
            for (int i = t; i < TR * a.pz; i += NT) {
                const int r = i / a.pz, c = i - r * a.pz;
                float z = 0.f;
                if (c < d && r0 + r < a.R) {
                    const float mu = Hh[r * psh + c], lv = Hh[r * psh + d + c];
                    z = __fadd_rn(__fmul_rn(ep[r * d + c], expf(0.5f * lv)), mu);
                    kl += -0.5 * ((double)lv - exp((double)lv) - (double)mu * (double)mu + 1.0);
                }
                Z[i] = z;
            }
            __syncthreads();
        }
        const float* Hin = VAE && l == a.vae_l ? sl + a.lz : sl + a.lh[l];
        float* Hout = sl + a.lh[l + 1];
        const int psin = VAE && l == a.vae_l ? a.pz : a.ps[l], pso = a.ps[l + 1];
        const bool last = l == L - 1;
        const float* H0row = sl + a.lh[0] + (k.rg * 16 + 4 * k.q) * a.ps[0];
        snet_forward_layer<TR>(k, y, sl, Hin, psin, Hout, pso, [&](sv4f& h, int col) {
            if (!last) return;
            // autoencoder loss on the spot: e = (y - xn) * range ; dY = scale * (y - xn) * range^2 * act'(y)
            const float rgv = col < y.out ? a.range[col] : 0.f;
            const sv4f dh = snet_actgrad4(y.act, h);
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                float g = 0.f;
                if (col < y.out && r0 + k.rg * 16 + 4 * k.q + v < a.R) {
                    const float x = H0row[v * a.ps[0] + col];
                    const float ev = (h[v] - x) * rgv;
                    sse += (double)ev * (double)ev;
                    g = a.scale * (h[v] - x) * rgv * rgv * dh[v];
                }
                h[v] = g;   // H_L now holds dZ_L
            }
        });
        __syncthreads();
        SNET_STAMP(3 + l);
    }
    // ---- squared error of the tile -> partial -> (ticket) the step's loss record
    {
        // waves by shuffles, the eight wave sums in wave order by one thread (a fixed order: deterministic)
        double* red = reinterpret_cast<double*>(sl + a.lred);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            sse += __shfl_down(sse, off, 64);
            if (VAE) kl += __shfl_down(kl, off, 64);
        }
        if (lane == 0) {
            red[wave] = sse;
            red[kSnetWaves + wave] = kl;
        }
        __syncthreads();
        if (t == 0) {
            double tot = red[0], ktot = red[kSnetWaves];
#pragma unroll
            for (int w = 1; w < kSnetWaves; ++w) {
                tot += red[w];
                ktot += red[kSnetWaves + w];
            }
            handoff_store(a.sse_part + blockIdx.x, tot);
            if (VAE) handoff_store(a.kl_part + blockIdx.x, ktot);
        }
    }
    SNET_STAMP(20);
    // ---- backward chain: dZ_l lives in the buffer of H_{l+1}; dZ_{l-1} is written over H_l once the weight gradient
    //      of layer l (which reads H_l) has been formed by every wave
    if (a.train) {
        for (int l = L - 1; l >= 0; --l) {
            const SnetLayer& y = a.l[l];
            const float* dZ = sl + a.lh[l + 1];
            float* Hin = sl + a.lh[l];
            const int psz = a.ps[l + 1], psh = a.ps[l];
            const float* Hw = VAE && l == a.vae_l ? sl + a.lz : Hin;   // input of this Linear (VAE: z for the first decoder Linear)
            const int psw = VAE && l == a.vae_l ? a.pz : psh;
            // input gradient first, kept in registers
            sv4f dg[kSnetMaxTiles];
            if (l > 0) snet_dgrad_layer<TR>(k, y, sl, dZ, psz, dg);
            SNET_STAMP(40 + l);
            snet_wgrad_partials<TR>(k, y, a.part, Hw, psw, dZ, psz);
            SNET_STAMP(48 + l);
            snet_bgrad_partials<TR>(k, y, a.part, dZ, psz);
            SNET_STAMP(21 + 2 * l);
            if (l == 0) break;
            __syncthreads();   // every wave is done reading H_l
            const int act_prev = a.l[l - 1].act, out_prev = a.l[l - 1].out;
            if (VAE && l == a.vae_l) {
                // dL/dz (no activation between z and this Linear) -> [dL/dmu | dL/dlv] over H_l = [mu | lv]: the thread of column
                // j < d owns columns j and d + j of its rows, columns [d, 2d) have no thread of their own, the padding is zeroed.
                const int d = a.vae_d;
                const float* ep = a.eps + ((int64_t)bj * a.R + r0) * d;
#pragma unroll
                for (int j = 0; j < kSnetMaxTiles; ++j) {
                    const int it = k.cg + j * SnetCoords<TR>::CG;
                    if (it < y.nk_in) {
                        const int col = it * 16 + k.n;
                        float* p = Hin + (k.rg * 16 + 4 * k.q) * psh + col;
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const int r = k.rg * 16 + 4 * k.q + v;
                            if (col < d) {
                                float gm = 0.f, gl = 0.f;
                                if (r0 + r < a.R) {
                                    const float mu = p[v * psh], lv = p[v * psh + d], e = ep[r * d + col], dz = dg[j][v];
                                    // the roundings spelt out (as for z above): left to the compiler, WHICH of gl's two products
                                    // is fused into the sum changes with the code around it, and with it the last bit
                                    gm = __fmaf_rn(a.beta_b, mu, dz);
                                    gl = __fmaf_rn(a.beta_b * 0.5f, expf(lv) - 1.f, __fmul_rn(dz * e * 0.5f, expf(0.5f * lv)));
                                }
                                p[v * psh] = gm;
                                p[v * psh + d] = gl;
                            } else if (col >= out_prev) {
                                p[v * psh] = 0.f;
                            }
                        }
                    }
                }
                __syncthreads();
                continue;
            }
            snet_dz_prev<TR>(k, y, act_prev, out_prev, Hin, psh, dg);
            __syncthreads();
        }
    }
    SNET_STAMP(60);
    // ---- last workgroup: total squared error in block order, loss record
    unsigned* flag = reinterpret_cast<unsigned*>(sl + a.lred);
    __syncthreads();
    const unsigned wgpb = a.nb > 1 ? (unsigned)a.wgpb : gridDim.x;
    if (!handoff_arrive_last(a.ticket + bj, wgpb, flag)) return;
    SNET_STAMP(61);
    if (t < 64) {
        const double* sp = a.sse_part + (int64_t)bj * wgpb;
        const double tot = wave_sum_in_order([&](int b) { return handoff_load(sp + b); }, (int)wgpb, t);
        double kl = 0.0;   // VAE: the KL partials, the same lane / shuffle order
        if (VAE) {
            const double* kp = a.kl_part + (int64_t)bj * wgpb;
            kl = wave_sum_in_order([&](int b) { return handoff_load(kp + b); }, (int)wgpb, t);
        }
        if (t == 0) {
            if (a.nb <= 1) a.stats[0] = tot;
            if (a.nb <= 1 && VAE) a.stats[1] = kl;
            if (a.log != nullptr) {   // (a data-parallel step logs after the all-reduce of the sum: ae_log_kernel)
                // a batched evaluation appends its records in batch order (loss_head.h: log_member): every batch's last arriver
                // reads the counter; the last of those moves it -- the VAE's batched pass leaves that to launch_log_advance
                const int slot0 = *a.log_count;
                const MemberLog ml = log_member(a.log, a.log_width, a.log_cap, bj);
                if (slot0 < ml.cap) ae_loss_record(ml.log + (int64_t)slot0 * a.log_width, tot, kl, a.Bg, a.l[0].in, a.beta, VAE);
                if (a.nb <= 1) {
                    *a.log_count = slot0 + 1;
                } else if (!VAE) {
                    asm volatile("s_waitcnt vmcnt(0) ; the counter has been read" ::: "memory");
                    log_advance_by_ticket(a.ticket + a.nb, a.nb, a.log_count, slot0);
                }
            }
        }
    }
}

struct SnetPlan {
    int tr_max;          // largest tile (32 or 16 rows) whose activation map fits in LDS behind the weight images; 16 always fits when 32 does
    int fl;              // LDS floats of the weight images
    SnetArgs base;       // layer table (the activation map is laid out per launch: it depends on the tile rows)
    float* part;         // gradient partials
    int64_t part_floats; // capacity
    int64_t per_wg;      // floats of one workgroup's partials over all layers (dense: sum out * in + out)
    unsigned long long* stamps;   // 64 words, or null (DCV_SNET_STAMPS=1)
    int2* stage_tab;     // device copy of the staging table
    double* ev_sse;      // batched evaluation: squared-error partials [batches][workgroups per batch] ...
    int64_t ev_sse_n;
    unsigned* ev_ticket; // ... and one ticket per batch + the one that moves the log counter (zero between launches)
    int64_t ev_ticket_n;
    double* kl_part;     // VAE: KL partials [workgroups of the launch] (kEvalWorkgroupsPerLaunch), or null
    int last_tr;         // tile rows of the last launch (dcv_debug_snet_tile_rows)
};

// Activation map of a TR-row tile behind the weight images (H_0 .. H_L, the reduction scratch); returns the LDS bytes, 0 when
// the tile does not fit
static size_t snet_ae_map(SnetArgs& a, int L, int fl, int TR) {
    for (int l = 1; l < L; ++l)
        if (a.l[l].pin != a.l[l - 1].pout) return 0;   // (always equal: both pad the same width)
    int f = snet_act_map(a.l, L, TR, fl, a.lh, a.ps);
    if (a.vae_l >= 0) {   // the z tile: the decoder's input, apart from the heads' output it is sampled from
        a.pz = a.l[a.vae_l].pin + 4;
        a.lz = f;
        f += TR * a.pz;
    }
    f = (f + 3) / 4 * 4;
    a.lred = f;
    f += 2 * kSnetThreads;   // kSnetThreads doubles
    return (size_t)f * sizeof(float) <= (size_t)160 * 1024 ? (size_t)f * sizeof(float) : 0;
}
// Rows per workgroup for batches of R rows.  16-row tiles shorten the latency chain of a workgroup; measured on one box
// (tools/dbg/ae_tr_probe.py, contiguous batches, us per training step, 16 | 32 rows): 54-16-8-2 autoencoder 27.0 | 28.5 at batch
// 128, 27.0 | 29.4 at 512, 28.2 | 29.8 at 2048, 30.8 | 30.3 at 4096; the C2 network 128-64-32-2: 31.1 | 35.7 at 128, 31.1 | 36.9
// at 512, 33.1 | 37.3 at 2048 (21 MB of partials and still ahead), 37.4 | 37.9 at 4096.  So: 16 rows up to 2048 rows (128
// workgroups), the larger tile beyond.  The choice depends on the rows of ONE batch only: a batched validation pass tiles its
// batches as the single steps would, so its records stay bit-equal to theirs.
static int snet_ae_pick_tr(const SnetPlan* pl, int64_t R) {
    static const int tr_env = (int)env_int("DCV_SNET_TR", 0);   // 16 | 32: force the rows per workgroup
    if ((tr_env == 16 || tr_env == 32) && tr_env <= pl->tr_max) return tr_env;
    if (pl->tr_max == 32) {
        if (cdiv(R, 16) <= 128) return 16;
    }
    return pl->tr_max;
}

// Builds the plan once per engine.  Not applicable (returns false): wide layers, dropout, a network that does not fit
// in LDS with at least 16-row tiles.
static bool snet_build(dcv_mlp* m) {
    if ((m->desc.model != DCV_MODEL_AE && m->desc.model != DCV_MODEL_VAE) || m->any_drop || snet_disabled()) return false;
    SnetPlan* pl = new (std::nothrow) SnetPlan();   // value-initialised: no buffer yet
    if (!pl) return false;
    m->snet = pl;   // from here on a half-built plan is released by snet_free
    SnetArgs& a = pl->base;
    a.L = m->L;
    a.vae_l = m->vae_d > 0 ? m->desc.latent_layer : -1;
    a.vae_d = m->vae_d;
    auto fail = [&] {
        snet_free(m);
        return false;
    };
    int64_t kl_n = 0, stamps_n = 0;
    if (m->vae_d > 0 && !snet_grow(&pl->kl_part, &kl_n, kEvalWorkgroupsPerLaunch)) return fail();
    std::vector<int2> tab;
    if (!snet_layout(m, a.l, tab, nullptr, pl->fl, pl->per_wg)) return fail();
    (void)snet_image_build(m);   // on failure the kernels keep the table-driven staging
    if (!snet_upload_table(tab, &pl->stage_tab)) return fail();
    a.stage_tab = pl->stage_tab;
    a.stage_n = (int)tab.size();
    for (int TR : {32, 16}) {
        SnetArgs tmp = a;
        if (snet_ae_map(tmp, m->L, pl->fl, TR) != 0) {
            pl->tr_max = TR;
            break;
        }
    }
    if (pl->tr_max == 0) return fail();
    // batched validation passes: partials and tickets for the bounds of dcv_mlp_eval_steps (33 KB); without them the
    // passes go batch by batch
    if (!snet_grow(&pl->ev_sse, &pl->ev_sse_n, kEvalWorkgroupsPerLaunch) || !snet_grow(&pl->ev_ticket, &pl->ev_ticket_n, (int64_t)kEvalBatchesPerLaunch + 1) ||
        hipMemset(pl->ev_ticket, 0, (size_t)pl->ev_ticket_n * sizeof(unsigned)) != hipSuccess) {
        (void)hipGetLastError();
        pl->ev_sse_n = pl->ev_ticket_n = 0;   // (the buffers go with the plan)
    }
    const char* e = getenv("DCV_SNET_STAMPS");
    if (e && e[0] == '1' && snet_grow(&pl->stamps, &stamps_n, 64)) (void)hipMemset(pl->stamps, 0, 64 * sizeof(unsigned long long));
    // the plan is built inside an engine's first step and the memsets above went to the null stream: they must have
    // landed before that step launches on the caller's stream, which need not wait for the null stream (dcv.h: all work
    // of an entry is on its stream).  Once per engine, next to the allocations.
    if (hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        return fail();
    }
    return true;
}

// ---- the global weight image: every weight / bias at its LDS-image offset, zero padding included, kept current by the
// optimiser kernels (OptArgs::img / img_idx) and rebuilt by dcv_mlp_set_params
__global__ __launch_bounds__(256) void snet_pack_kernel(const float* __restrict__ params, const int* __restrict__ idx, int64_t n, float* __restrict__ img) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int j = idx[i];
        if (j >= 0) img[j] = params[i];
    }
}
bool snet_image_build(dcv_mlp* m) {
    static const bool off = env_is("DCV_SNET_IMG", '0');
    if (off) return false;
    if (m->snet_img != nullptr) return true;
    SnetLayer ly[DCV_MAX_LAYERS];
    std::vector<int2> tab;
    std::vector<int> idx;
    int fl = 0;
    int64_t per_wg = 0;
    if (!snet_layout(m, ly, tab, nullptr, fl, per_wg, &idx)) return false;
    for (int l = 0; l < m->L; ++l)   // 16-byte copies: every image row must start on a 16-byte boundary (pws and pout are multiples of 4)
        if ((ly[l].lw & 3) || (ly[l].lb & 3)) return false;
    float* img = nullptr;
    int* didx = nullptr;
    const size_t fpad = ((size_t)fl + 255) / 256 * 256;
    if (hipMalloc(reinterpret_cast<void**>(&img), fpad * sizeof(float)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&didx), idx.size() * sizeof(int)) != hipSuccess ||
        hipMemset(img, 0, fpad * sizeof(float)) != hipSuccess ||
        hipMemcpy(didx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (img) (void)hipFree(img);
        if (didx) (void)hipFree(didx);
        return false;
    }
    m->snet_img = img;
    m->snet_img_idx = didx;
    m->snet_img_floats = fl;
    if (snet_image_repack(m, nullptr) != DCV_OK || hipDeviceSynchronize() != hipSuccess) {
        (void)hipGetLastError();
        snet_image_free(m);
        return false;
    }
    return true;
}
int snet_image_repack(dcv_mlp* m, hipStream_t s) {
    if (m->snet_img == nullptr) return DCV_OK;
    int64_t blocks = cdiv(m->n_params, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(snet_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)m->params, (const int*)m->snet_img_idx, m->n_params, m->snet_img);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
void snet_image_free(dcv_mlp* m) {
    if (m->snet_img) (void)hipFree(m->snet_img);
    if (m->snet_img_idx) (void)hipFree(m->snet_img_idx);
    m->snet_img = nullptr;
    m->snet_img_idx = nullptr;
    m->snet_img_floats = 0;
}

void snet_free(dcv_mlp* m) {
    SnetPlan* pl = static_cast<SnetPlan*>(m->snet);
    if (!pl) return;
    if (pl->part) (void)hipFree(pl->part);
    if (pl->stamps) (void)hipFree(pl->stamps);
    if (pl->stage_tab) (void)hipFree(pl->stage_tab);
    if (pl->ev_sse) (void)hipFree(pl->ev_sse);
    if (pl->ev_ticket) (void)hipFree(pl->ev_ticket);
    if (pl->kl_part) (void)hipFree(pl->kl_part);
    delete pl;
    m->snet = nullptr;
}

int snet_ae_last_tile_rows(const dcv_mlp* m) {
    const SnetPlan* pl = static_cast<const SnetPlan*>(m->snet);
    return pl ? pl->last_tr : 0;
}

// Rows per workgroup the fused autoencoder kernel takes for batches of R rows (R = 0: its largest tile); the plan is built on
// first use; 0: the fused form does not apply.
int snet_ae_tile_rows(dcv_mlp* m, int64_t R) {
    if (!snet_plan_ready(m->snet, m->snet_tried, [&] { return snet_build(m); })) return 0;
    const SnetPlan* pl = static_cast<SnetPlan*>(m->snet);
    return R > 0 ? snet_ae_pick_tr(pl, R) : pl->tr_max;
}

// One fused step of the autoencoder over `R` rows (train != 0: gradient partials are left for the reduction, whose
// descriptors are filled into `ra`).  Returns 1 when the fused form does not apply (the caller takes the layer-by-layer
// path), DCV_OK when the launch was enqueued.
// nb > 1 (evaluation only): nb batches of R rows each in the one launch -- batch j = the logical rows [j * R, (j + 1) * R) of
// `rm` -- with one loss record per batch, appended in batch order.
int snet_ae_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const RowMap& rm, int64_t R, int64_t batch, int train, ReduceArgsView* ra,
                 hipStream_t s, bool write_log, int nb) {
    static const int64_t kMaxPartBytes = 96ll << 20;
    if (snet_ae_tile_rows(m) == 0) return 1;
    SnetPlan* pl = static_cast<SnetPlan*>(m->snet);
    const int TR = snet_ae_pick_tr(pl, R);
    const int64_t wgpb = cdiv(R, TR);
    if (wgpb > m->spart_blocks || wgpb * pl->per_wg * (int64_t)sizeof(float) > kMaxPartBytes || wgpb > 512) return 1;   // large batches: the tiled products are the better engine
    if (nb < 1 || (nb > 1 && (train || !write_log))) return 1;
    const int64_t nwg = wgpb * nb;
    if (nb > 1 && (nwg > pl->ev_sse_n || nb + 1 > pl->ev_ticket_n)) return 1;   // (sized by snet_build for the bounds of dcv_mlp_eval_steps)
    if (m->vae_d > 0 && (pl->kl_part == nullptr || nwg > kEvalWorkgroupsPerLaunch || m->eps_cur == nullptr)) return 1;
    const int64_t part_need = nwg * pl->per_wg + 8 * (int64_t)m->L;   // + the alignment padding of the items
    if (train && !snet_grow(&pl->part, &pl->part_floats, part_need)) return 1;
    SnetArgs a = pl->base;
    const size_t lds_bytes = snet_ae_map(a, m->L, pl->fl, TR);
    if (lds_bytes == 0) return 1;
    snet_partials_layout(a.l, m->L, nwg, pl->part, ra);
    a.params = m->params;
    a.img = m->snet_img;
    a.img_floats = m->snet_img_floats;
    a.Xn = Xn_d;
    a.ld = ld;
    a.rows = rm;
    a.R = R;
    a.nb = nb;
    a.wgpb = (int)wgpb;
    a.range = m->feat_range;
    a.scale = (float)(2.0 / ((double)batch * (double)m->desc.dims[0]));
    a.train = train;
    a.part = pl->part;
    a.sse_part = nb > 1 ? pl->ev_sse : m->spart;
    a.ticket = nb > 1 ? pl->ev_ticket : m->ticket;
    a.stats = m->stats;
    a.Bg = (double)batch;
    a.log = write_log ? m->log : nullptr;
    a.log_count = m->log_count;
    a.log_cap = m->log_cap;
    a.log_width = m->log_width;
    a.eps = m->eps_cur;
    a.beta = m->kl_beta;
    a.beta_b = (float)(m->kl_beta / (double)batch);
    a.kl_part = pl->kl_part;
    a.stamps = pl->stamps;
    pl->last_tr = TR;
    static int attr_state[4] = {0, 0, 0, 0};   // per kernel instantiation (snet_launch)
    auto launch = [&](auto kern) -> int {
        return snet_launch(kern, attr_state[(TR == 32 ? 0 : 1) + (a.vae_l >= 0 ? 2 : 0)], 160 * 1024, lds_bytes, a, nwg, s);
    };
    if (a.vae_l >= 0) {
        const int rc = TR == 32 ? launch(snet_ae_kernel<32, true>) : launch(snet_ae_kernel<16, true>);
        if (rc == DCV_OK && nb > 1 && a.log != nullptr) return launch_log_advance(m->log_count, nb, s);
        return rc;
    }
    return TR == 32 ? launch(snet_ae_kernel<32, false>) : launch(snet_ae_kernel<16, false>);
}

}  // namespace dcv

// diagnostic (tools/dbg/snet_probe.py; not part of include/dcv.h): the 64 phase stamps of the last fused launch
// (s_memrealtime ticks of 10 ns), 0 where not taken; needs DCV_SNET_STAMPS=1 at engine creation
extern "C" int dcv_debug_snet_stamps(dcv_mlp* m, unsigned long long* out_h) {
    using namespace dcv;
    if (!m || !out_h) return DCV_EINVAL;
    SnetPlan* pl = static_cast<SnetPlan*>(m->snet);
    if (!pl || !pl->stamps) return 1;
    DCV_CHECK_HIP(hipDeviceSynchronize());
    DCV_CHECK_HIP(hipMemcpy(out_h, pl->stamps, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return DCV_OK;
}

// diagnostic (tests; not part of include/dcv.h): rows per workgroup of the last fused small-network launch (16 / 32 / 64 / 128),
// 0 when the last step or forward ran layer by layer
extern "C" int dcv_debug_snet_tile_rows(const dcv_mlp* m) {
    using namespace dcv;
    if (!m) return DCV_EINVAL;
    if (m->last_path == 1) return snet_ae_last_tile_rows(m);
    if (m->last_path == 2) return snet_dt_last_tile_rows(m);
    return 0;
}

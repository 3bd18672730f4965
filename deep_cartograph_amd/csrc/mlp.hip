// MLP engine: Deep-TICA and autoencoder training / inference on the FP32 MFMA block engine.
//
// A step never materialises the batch: the first layer gathers its rows straight from the
// resident, pre-normalised feature matrix through a RowMap (x_t rows, then the same samples
// `lag` rows later for Deep-TICA).  Every Linear layer is three products on the same engine
//   forward  H_l  = act(In_l W_l^T + b_l)                      NT, fused bias + activation
//   dgrad    dZ_{l-1} = (dZ_l W_l) * act'(H_{l-1})             NN, fused activation gradient
//   wgrad    dW_l = dZ_l^T In_l                                TN, split over the batch rows
// wgrad split partials and the bias column sums are folded in a fixed order by one reduction
// kernel (deterministic), Adam is one more launch.  The d x d TICA algebra of the Deep-TICA
// loss runs in float64 on the device from batch statistics that a data-parallel caller
// all-reduces, so nothing returns to the host inside an epoch.
//
// This unit: lifecycle and accessors, the layer-by-layer forward and backward, the single-step entry points.  mlp_opt.hip:
// optimisers and gradient reduction; mlp_heads.hip: loss heads; mlp_passes.hip: the passes built on the steps.
#include "mlp_state.h"
#include "reduce_quad.h"
#include <new>
#include <math.h>
#include <utility>

using namespace dcv;

namespace dcv {

// ------------------------------------------------------------------ small kernels
// partial column sums of dZ (rows x n): part[block][n], one block per kColsumRows rows.  Threads are
// laid out (row group, column): wide matrices give every thread one column, narrow ones (the d
// outputs of the last layer) put many row groups on one column and combine them through LDS.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ Z, int64_t rows, int n, int64_t ld,
                                                     float* __restrict__ part) {
    __shared__ float red[256];
    const int64_t r0 = (int64_t)blockIdx.x * kColsumRows;
    const int64_t r1 = r0 + kColsumRows < rows ? r0 + kColsumRows : rows;
    const int t = threadIdx.x;
    const int cols = n < 256 ? n : 256;   // columns handled per pass
    const int groups = 256 / cols;        // row groups per column
    const int c_in = t % cols, g = t / cols;
    for (int c0 = 0; c0 < n; c0 += cols) {
        const int c = c0 + c_in;
        float s = 0.f;
        if (g < groups && c < n) {
            // eight loads in flight, added in row order (the same sum as a serial walk, without its dependent round trips)
            for (int64_t rb = r0 + g; rb < r1; rb += 8 * (int64_t)groups) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t r = rb + (int64_t)u * groups;
                    v[u] = r < r1 ? Z[r * ld + c] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
        }
        red[t] = s;
        __syncthreads();
        if (g == 0 && c < n) {
            float tot = 0.f;
            for (int q = 0; q < groups; ++q) tot += red[q * cols + c_in];
            part[(int64_t)blockIdx.x * n + c] = tot;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ variational autoencoder: reparameterisation
// H = [mu | lv] (2d columns, the two heads of Linear latent_layer - 1), eps [R][d] dense:
//   z = eps * exp(lv / 2) + mu                       (torch: randn_like(mu) * torch.exp(0.5 * log_var) + mu)
//   part[block] = sum over the block's rows of -0.5 * sum_j (lv - exp(lv) - mu^2 + 1)   (float64, fixed tree order)
__global__ __launch_bounds__(kVaeRows) void vae_sample_kernel(const float* __restrict__ H, int64_t ldh, int64_t R, int d,
                                                             const float* __restrict__ eps, float* __restrict__ Z, int64_t ldz,
                                                             double* __restrict__ part) {
    __shared__ double red[kVaeRows];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kVaeRows + t;
    double kl = 0.0;
    if (r < R) {
        for (int j = 0; j < d; ++j) {
            const float mu = H[r * ldh + j], lv = H[r * ldh + d + j];
            Z[r * ldz + j] = __fadd_rn(__fmul_rn(eps[r * d + j], expf(0.5f * lv)), mu);
            kl += (double)lv - exp((double)lv) - (double)mu * (double)mu + 1.0;
        }
        kl *= -0.5;
    }
    red[t] = kl;
    __syncthreads();
    for (int off = kVaeRows / 2; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

// in place: G holds dL/dz in columns [0, d) of each row; out: [dL/dmu | dL/dlv] in columns [0, 2d)
//   dmu = dz + beta * mu / B,  dlv = dz * eps * 0.5 * exp(lv / 2) + beta * 0.5 * (exp(lv) - 1) / B
__global__ __launch_bounds__(kVaeRows) void vae_sample_backward_kernel(const float* __restrict__ H, int64_t ldh, int64_t R, int d,
                                                                      const float* __restrict__ eps, float* __restrict__ G, int64_t ldg,
                                                                      float beta_over_b) {
    const int64_t r = (int64_t)blockIdx.x * kVaeRows + threadIdx.x;
    if (r >= R) return;
    float dz[8];
    for (int j = 0; j < d; ++j) dz[j] = G[r * ldg + j];
    for (int j = 0; j < d; ++j) {
        const float mu = H[r * ldh + j], lv = H[r * ldh + d + j];
        G[r * ldg + j] = dz[j] + beta_over_b * mu;
        G[r * ldg + d + j] = dz[j] * eps[r * d + j] * 0.5f * expf(0.5f * lv) + beta_over_b * 0.5f * (expf(lv) - 1.f);
    }
}

// test hook: the keep / (1 - p) multipliers of a layer's dropout for rows [0, rows)
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* __restrict__ out, int64_t rows, int width, DropCfg drop) {
    const int q4 = (width + 3) / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < rows * q4; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / q4;
        const int c = (int)(i - r * q4) * 4;
        const float4 k = drop.thr != 0u ? drop.mult(r, c) : make_float4(1.f, 1.f, 1.f, 1.f);
        float* o = out + r * width + c;
        o[0] = k.x;
        if (c + 1 < width) o[1] = k.y;
        if (c + 2 < width) o[2] = k.z;
        if (c + 3 < width) o[3] = k.w;
    }
}

// wgrad split plan: enough workgroups to fill the chip twice, chunks a multiple of 32 rows
static void wgrad_plan(int out, int in, int64_t rows, int64_t* k_chunk, int64_t* splits) {
    const int64_t tiles = (out <= 32 ? 1 : cdiv(out, 128)) * (in <= 32 ? 1 : cdiv(in, 128));
    int64_t want = cdiv(2 * (int64_t)num_cus(), tiles);
    int64_t max_by_rows = cdiv(rows, 256);
    // Small batches.  When 64 x 64 tiles reach two workgroups per CU with a split count the rows allow, take them
    // (pick_cfg<kTN> follows: fewer than one 128 x 128 workgroup per CU): measured on the 256 x 512 x 8202 product, 16 chunks
    // of 64 x 64 tiles 21.9 us against 29 chunks of 128 x 128 tiles 23.7 -- and 16 slabs instead of 29 to write and reduce; a
    // multiple of 8 chunks lets the XCD map keep a chunk's rows in one L2.  Round 4 tried the same plan where the rows would
    // allow the 128 x 128 one but the chunks stay short (<= 1024 rows: the 16 384 rows of a gathered 8192-pair batch give 64
    // slabs of 512 KB per step -- 32 MB written and re-read by the reduction, 11.4 us -- where 16 chunks of 64 x 64 tiles leave
    // 8 MB): the reduction fell to 7.0 us, but the GATHERED weight gradient went from 38.7 to 60.0 us (per-thread 64-bit row
    // pointers: four times the stage loads per flop of the 128 x 128 tile) -- kept behind DCV_WGRAD_Q=1, off by default.
    static const bool q_wide = env_is("DCV_WGRAD_Q", '1');   // opt-in: see below
    const int64_t tiles_q = cdiv(out, 64) * cdiv(in, 64);
    const int64_t want_q = cdiv(cdiv(2 * (int64_t)num_cus(), tiles_q), 8) * 8;
    if (out > 32 && in > 32 && want_q <= max_by_rows) {
        int64_t kc = cdiv(cdiv(rows, want_q), 32) * 32;
        if (cdiv(rows, kc) % 8 != 0) kc = cdiv(rows, want_q);   // ragged chunk ends (the stage tail goes through registers)
        if (tiles * cdiv(rows, kc) <= (int64_t)num_cus() / 2 &&   // pick_cfg<kTN>'s condition for 64 x 64 tiles
            (want > max_by_rows || (q_wide && kc <= 1024))) {
            *k_chunk = kc;
            *splits = cdiv(rows, kc);
            return;
        }
    }
    if (want > max_by_rows) {
        // row-limited: a split count that is a multiple of 8 keeps tiles x splits on whole multiples of the CU count (33
        // splits x 8 tiles = 264 workgroups cost 1.6 x of 256: the 8 extra share SIMDs with 8 others)
        want = max_by_rows >= 8 ? max_by_rows / 8 * 8 : max_by_rows;
    }
    if (want < 1) want = 1;
    int64_t kc = cdiv(cdiv(rows, want), 32) * 32;
    *k_chunk = kc;
    *splits = cdiv(rows, kc);
}

static void mlp_free(dcv_mlp* m) {
    if (!m) return;
    snet_free(m);
    snet_dt_free(m);
    snet_image_free(m);
    auto f = [](void* p) { if (p) (void)hipFree(p); };
    f(m->params); f(m->grads); f(m->adam_m); f(m->adam_v); f(m->opt_aux); f(m->dZ[0]); f(m->dZ[1]); f(m->stats); f(m->gradp);
    f(m->spart); f(m->log); f(m->log_count); f(m->ticket); f(m->feat_range); f(m->ident); f(m->zeros_d); f(m->ones_d); f(m->proj_ws);
    f(m->vae_z); f(m->vae_kpart);
    for (auto& l : m->layers) { f(l.H); f(l.slab); f(l.bpart); f(l.mask); f(l.Y); f(l.rm); f(l.rv); f(l.bn_stat); f(l.bn_part); f(l.bn_gpart); f(l.bn_bpart); }
    g_launch_ev = LaunchEvents{};   // no stale offer of events that are about to be destroyed
    g_launch_taken = nullptr;
    for (hipEvent_t e : m->prof_ev) (void)hipEventDestroy(e);
    f(m->tail.ws); f(m->tail.cnt); f(m->eval_ws.base);
    for (int i = 0; i < 4; ++i) if (m->gexec[i]) (void)hipGraphExecDestroy(m->gexec[i]);
    delete m;
}

// running statistics of a freshly constructed BatchNorm1d: mean 0, variance 1, no batches tracked
static int reset_bn_state(dcv_mlp* m, hipStream_t s) {
    for (auto& p : m->layers) {
        if (!p.bn) continue;
        DCV_CHECK_HIP(hipMemsetAsync(p.rm, 0, (size_t)p.out * sizeof(float), s));
        launch_fill(p.rv, (int64_t)p.out, 1.f, 1, 256, s);
        DCV_CHECK_LAUNCH();
        p.bn_batches = 0;
    }
    return DCV_OK;
}

static int create_validate(const dcv_mlp_desc* desc) {
    const int L = desc->n_layers;
    DCV_REQUIRE(desc->model == DCV_MODEL_DEEPTICA || desc->model == DCV_MODEL_AE || desc->model == DCV_MODEL_VAE, "dcv_mlp_create: unknown model %d",
                desc->model);
    DCV_REQUIRE(L >= 1 && L <= DCV_MAX_LAYERS, "dcv_mlp_create: n_layers=%d out of range", L);
    for (int l = 0; l <= L; ++l) DCV_REQUIRE(desc->dims[l] >= 1, "dcv_mlp_create: dims[%d]=%d", l, desc->dims[l]);
    for (int l = 0; l < L; ++l)
        DCV_REQUIRE(desc->act[l] >= DCV_ACT_NONE && desc->act[l] <= DCV_ACT_CUSTOM_SIGMOID, "dcv_mlp_create: act[%d]=%d unsupported", l, desc->act[l]);
    for (int l = 0; l < L; ++l)
        DCV_REQUIRE(desc->dropout[l] >= 0.f && desc->dropout[l] < 1.f, "dcv_mlp_create: dropout[%d]=%g outside [0, 1)", l, (double)desc->dropout[l]);
    DCV_REQUIRE(desc->optimizer >= DCV_OPT_ADAM && desc->optimizer <= DCV_OPT_RPROP, "dcv_mlp_create: optimizer %d unknown", desc->optimizer);
    DCV_REQUIRE(desc->max_batch >= 1, "dcv_mlp_create: max_batch=%d", desc->max_batch);
    if (desc->model == DCV_MODEL_DEEPTICA) {
        DCV_REQUIRE(desc->dims[L] <= kMaxTicaDim, "dcv_mlp_create: Deep-TICA output dimension %d > %d", desc->dims[L], kMaxTicaDim);
        DCV_REQUIRE(desc->lag >= 0, "dcv_mlp_create: lag=%d", desc->lag);
    } else {
        DCV_REQUIRE(desc->dims[L] == desc->dims[0], "dcv_mlp_create: autoencoder must map F=%d back to F (got %d)", desc->dims[0], desc->dims[L]);
        DCV_REQUIRE(desc->latent_layer >= 1 && desc->latent_layer < L, "dcv_mlp_create: latent_layer=%d", desc->latent_layer);
        DCV_REQUIRE(desc->dims[desc->latent_layer] <= 16, "dcv_mlp_create: latent dimension %d > 16", desc->dims[desc->latent_layer]);
        if (desc->model == DCV_MODEL_VAE) {
            const int h = desc->latent_layer - 1;   // the two heads, concatenated: [mean | log-variance]
            DCV_REQUIRE(desc->dims[desc->latent_layer] % 2 == 0 && desc->dims[desc->latent_layer] <= 16,
                        "dcv_mlp_create: VAE head layer %d must output 2 * d <= 16 columns (got %d)", h, desc->dims[desc->latent_layer]);
            DCV_REQUIRE(desc->act[h] == DCV_ACT_NONE && !(desc->dropout[h] > 0.f) && !desc->batchnorm[h],
                        "dcv_mlp_create: the VAE heads (Linear %d) take no activation, dropout or batch normalisation", h);
        }
    }
    return DCV_OK;
}
// width of the projection behind the network (dcv_mlp_infer): latent dimension of an autoencoder, else the output dimension
static int proj_dim(const dcv_mlp* m) {
    return m->desc.model == DCV_MODEL_AE ? m->desc.dims[m->desc.latent_layer] : m->desc.model == DCV_MODEL_VAE ? m->vae_d : m->d_out;
}
// every layer's place in the flat parameter buffer, its strides and its weight-gradient split capacity; the sizes that follow
static void plan_layers(dcv_mlp* m) {
    const dcv_mlp_desc* desc = &m->desc;
    const int L = m->L;
    m->layers.resize(L);
    int64_t off = 0;
    int maxdim = 0;
    for (int l = 0; l < L; ++l) {
        LayerPlan& p = m->layers[l];
        p.in = m->vae_d > 0 && l == desc->latent_layer ? m->vae_d : desc->dims[l];   // VAE: the first decoder Linear reads z (d columns)
        p.out = desc->dims[l + 1];
        p.act = desc->act[l];
        p.w_off = off;
        off += align_up((size_t)p.in * p.out, 4);
        p.b_off = off;
        off += align_up((size_t)p.out, 4);
        p.bn = desc->batchnorm[l] ? 1 : 0;
        if (p.bn) {
            p.g_off = off;
            off += align_up((size_t)p.out, 4);
            p.be_off = off;
            off += align_up((size_t)p.out, 4);
            m->any_bn = true;
        }
        p.ldh = align_up((size_t)p.out, 4);
        if (p.out > maxdim) maxdim = p.out;
        wgrad_plan(p.out, p.in, m->rows_cap, &p.k_chunk_cap, &p.max_splits);
        // a smaller batch may use smaller chunks; bound the splits by the 256-row floor
        p.max_splits = cdiv(m->rows_cap, 256) > p.max_splits ? p.max_splits : cdiv(m->rows_cap, 256);
        if (p.max_splits < 1) p.max_splits = 1;
        if (l == L - 1 && p.out <= 8) {   // the fused backward of a narrow last layer writes one partial per block (head_plan)
            int64_t hb = 4 * (int64_t)num_cus();
            if (hb > cdiv(m->rows_cap, 32)) hb = cdiv(m->rows_cap, 32);
            if (hb > p.max_splits) p.max_splits = hb;
        }
    }
    m->n_params = off;
    m->ld_dz = align_up((size_t)maxdim, 4);
    const int d = m->d_out;
    m->stats_len = desc->model == DCV_MODEL_DEEPTICA ? 2 * d + 2 * d * d : desc->model == DCV_MODEL_VAE ? 2 : 1;
    m->log_width = desc->model == DCV_MODEL_DEEPTICA ? 2 + 2 * d * d + d : desc->model == DCV_MODEL_VAE ? 4 : 2;
    m->spart_blocks = desc->model == DCV_MODEL_DEEPTICA ? (int)cdiv(desc->max_batch, kStatBlockRows) : (int)cdiv(m->rows_cap, kSseRows);
}
// device buffers, the layers' first (the order fixes the addresses); the first failure stops it, the caller frees what exists
static int alloc_buffers(dcv_mlp* m) {
    const dcv_mlp_desc* desc = &m->desc;
    int rc = DCV_OK;
    for (int l = 0; l < m->L && rc == DCV_OK; ++l) {
        LayerPlan& p = m->layers[l];
        rc = dmalloc(&p.H, (size_t)m->rows_cap * p.ldh);
        if (rc == DCV_OK) rc = dmalloc(&p.slab, (size_t)p.max_splits * p.in * p.out);
        if (rc == DCV_OK) rc = dmalloc(&p.bpart, (size_t)cdiv(m->rows_cap, 32) * p.out);  // row tiles of the dgrad epilogue can be as short as 32
        if (rc == DCV_OK && p.bn) {
            const size_t nblk = (size_t)cdiv(m->rows_cap, 256) + 2;
            rc = dmalloc(&p.Y, (size_t)m->rows_cap * p.ldh);
            if (rc == DCV_OK) rc = dmalloc(&p.rm, (size_t)p.out);
            if (rc == DCV_OK) rc = dmalloc(&p.rv, (size_t)p.out);
            if (rc == DCV_OK) rc = dmalloc(&p.bn_stat, (size_t)4 * p.out);
            if (rc == DCV_OK) rc = dmalloc(&p.bn_part, nblk * 2 * p.out);
            if (rc == DCV_OK) rc = dmalloc(&p.bn_gpart, nblk * p.out);
            if (rc == DCV_OK) rc = dmalloc(&p.bn_bpart, nblk * p.out);
        }
        if (rc == DCV_OK && l + 1 < m->L && (p.act == DCV_ACT_RELU || p.act == DCV_ACT_LEAKY_RELU))   // one bit per element, whole tiles
            rc = dmalloc(&p.mask, (size_t)((m->rows_cap + 128) * (int64_t)(p.out + 128)) / 64 + 64);
    }
    const int dl = proj_dim(m);
    if (rc == DCV_OK) rc = dmalloc(&m->params, (size_t)m->n_params);
    if (rc == DCV_OK) rc = dmalloc(&m->grads, (size_t)m->n_params);
    if (rc == DCV_OK) rc = dmalloc(&m->adam_m, (size_t)m->n_params);
    if (rc == DCV_OK) rc = dmalloc(&m->adam_v, (size_t)m->n_params);
    if (rc == DCV_OK && (((desc->optimizer == DCV_OPT_ADAM || desc->optimizer == DCV_OPT_ADAMW) && desc->amsgrad) ||
                         (desc->optimizer == DCV_OPT_RMSPROP && desc->centered)))
        rc = dmalloc(&m->opt_aux, (size_t)m->n_params);
    if (rc == DCV_OK) rc = dmalloc(&m->dZ[0], (size_t)m->rows_cap * m->ld_dz);
    if (rc == DCV_OK) rc = dmalloc(&m->dZ[1], (size_t)m->rows_cap * m->ld_dz);
    if (rc == DCV_OK) rc = dmalloc(&m->stats, (size_t)m->stats_len);
    if (rc == DCV_OK) rc = dmalloc(&m->gradp, (size_t)(2 * kMaxTicaDim + 2 * kMaxTicaDim * kMaxTicaDim));
    if (rc == DCV_OK) rc = dmalloc(&m->spart, (size_t)m->spart_blocks * m->stats_len);   // ticketed partials: handoff.h
    if (rc == DCV_OK) rc = dmalloc(&m->log_count, 1);
    if (rc == DCV_OK) rc = dmalloc(&m->ticket, 4);
    if (rc == DCV_OK) rc = dmalloc(&m->feat_range, (size_t)desc->dims[0]);
    if (rc == DCV_OK && m->vae_d > 0) rc = dmalloc(&m->vae_z, (size_t)m->rows_cap * m->ld_z);
    if (rc == DCV_OK && m->vae_d > 0) rc = dmalloc(&m->vae_kpart, (size_t)cdiv(m->rows_cap, kVaeRows));
    if (rc == DCV_OK) rc = dmalloc(&m->ident, (size_t)dl * dl);
    if (rc == DCV_OK) rc = dmalloc(&m->zeros_d, (size_t)dl);
    if (rc == DCV_OK) rc = dmalloc(&m->ones_d, (size_t)dl);
    m->proj_ws_bytes = dcv_project_linear_workspace(m->rows_cap, dl, dl);
    if (rc == DCV_OK) rc = dmalloc(reinterpret_cast<char**>(&m->proj_ws), m->proj_ws_bytes);
    return rc;
}
// zero parameters, a fresh optimiser and fresh normalisations, the constants of the inference projection
static int init_device_state(dcv_mlp* m) {
    const int dl = proj_dim(m);
    hipError_t e = hipMemset(m->params, 0, m->n_params * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->grads, 0, m->n_params * sizeof(float));
    if (e == hipSuccess && reset_opt_state(m, nullptr) != DCV_OK) e = hipErrorUnknown;
    if (e == hipSuccess) e = hipMemset(m->log_count, 0, sizeof(int));
    if (e == hipSuccess) e = hipMemset(m->ticket, 0, 4 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(m->zeros_d, 0, dl * sizeof(float));
    if (e == hipSuccess) e = hipMemset(m->ident, 0, (size_t)dl * dl * sizeof(float));
    if (e == hipSuccess) {
        launch_fill(m->ones_d, (int64_t)dl, 1.f, 1, 64, nullptr);
        launch_fill(m->feat_range, (int64_t)m->desc.dims[0], 1.f, 4, 256, nullptr);
        std::vector<float> eye((size_t)dl * dl, 0.f);
        for (int i = 0; i < dl; ++i) eye[(size_t)i * dl + i] = 1.f;
        e = hipMemcpy(m->ident, eye.data(), eye.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        for (auto& p : m->layers)
            if (p.bn) launch_fill(m->params + p.g_off, (int64_t)p.out, 1.f, 1, 256, nullptr);   // BatchNorm1d: weight 1, bias 0
        if (reset_bn_state(m, nullptr) != DCV_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess) (void)alloc_tail_ws(&m->tail, 8);   // up to 8 column tiles; on failure the tail cut stays off
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) return DCV_OK;
    set_error("dcv_mlp_create: initialisation failed: %s", hipGetErrorString(e));
    return DCV_EHIP;
}

}  // namespace dcv

extern "C" int dcv_mlp_create(const dcv_mlp_desc* desc, dcv_mlp** out) {
    DCV_REQUIRE(desc && out, "dcv_mlp_create: null argument");
    *out = nullptr;
    int rc = create_validate(desc);
    if (rc) return rc;
    dcv_mlp* m = new (std::nothrow) dcv_mlp();   // value-initialised: every member starts as zero / null / false or as mlp_state.h says
    DCV_REQUIRE(m, "dcv_mlp_create: out of host memory");
    m->desc = *desc;
    m->L = desc->n_layers;
    m->d_out = desc->dims[m->L];
    m->rows_cap = desc->model == DCV_MODEL_DEEPTICA ? 2 * (int64_t)desc->max_batch : desc->max_batch;
    m->lr = desc->lr;
    m->momentum_rt = (desc->optimizer == DCV_OPT_ADAM || desc->optimizer == DCV_OPT_ADAMW || desc->optimizer == DCV_OPT_ADAMAX ||
                      desc->optimizer == DCV_OPT_NADAM || desc->optimizer == DCV_OPT_RADAM) ? desc->beta1 : desc->momentum;
    for (int l = 0; l < m->L; ++l) m->any_drop = m->any_drop || desc->dropout[l] > 0.f;
    m->vae_d = desc->model == DCV_MODEL_VAE ? desc->dims[desc->latent_layer] / 2 : 0;
    m->ld_z = align_up((size_t)(m->vae_d > 0 ? m->vae_d : 1), 4);
    static const bool graph_env = env_is("DCV_GRAPH", '1');
    m->graph_on = graph_env;
    plan_layers(m);
    rc = alloc_buffers(m);
    if (rc == DCV_OK) rc = init_device_state(m);
    if (rc != DCV_OK) {
        mlp_free(m);
        return rc;
    }
    *out = m;
    return DCV_OK;
}

extern "C" void dcv_mlp_destroy(dcv_mlp* m) { mlp_free(m); }
extern "C" int64_t dcv_mlp_num_params(const dcv_mlp* m) { return m ? m->n_params : 0; }
extern "C" int64_t dcv_mlp_param_offset(const dcv_mlp* m, int32_t layer, int32_t which) {
    if (!m || layer < 0 || layer >= m->L) return -1;
    if (which == 2) return m->layers[layer].g_off;    // weight / bias of the batch normalisation behind the layer, -1 without one
    if (which == 3) return m->layers[layer].be_off;
    return which == 0 ? m->layers[layer].w_off : m->layers[layer].b_off;
}
extern "C" float* dcv_mlp_params(dcv_mlp* m) { return m ? m->params : nullptr; }
extern "C" float* dcv_mlp_grads(dcv_mlp* m) { return m ? m->grads : nullptr; }
extern "C" double* dcv_mlp_stats(dcv_mlp* m) { return m ? m->stats : nullptr; }
extern "C" int32_t dcv_mlp_stats_len(const dcv_mlp* m) { return m ? m->stats_len : 0; }
extern "C" int32_t dcv_mlp_log_width(const dcv_mlp* m) { return m ? m->log_width : 0; }

extern "C" int dcv_mlp_set_params(dcv_mlp* m, const float* params_h, void* stream) {
    DCV_REQUIRE(m && params_h, "dcv_mlp_set_params: null argument");
    hipStream_t s = as_stream(stream);
    DCV_CHECK_HIP(hipMemcpyAsync(m->params, params_h, m->n_params * sizeof(float), hipMemcpyHostToDevice, s));
    int rc = reset_opt_state(m, s);
    if (rc == DCV_OK) rc = reset_bn_state(m, s);
    if (rc == DCV_OK) rc = snet_image_repack(m, s);   // the fused small-network kernels' weight image follows the parameters
    if (rc) return rc;
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    return DCV_OK;
}

extern "C" int dcv_mlp_get_params(dcv_mlp* m, float* params_h, void* stream) {
    DCV_REQUIRE(m && params_h, "dcv_mlp_get_params: null argument");
    hipStream_t s = as_stream(stream);
    DCV_CHECK_HIP(hipMemcpyAsync(params_h, m->params, m->n_params * sizeof(float), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    return DCV_OK;
}

extern "C" int dcv_mlp_bn_state(dcv_mlp* m, int32_t layer, float* running_mean_h, float* running_var_h, int64_t* num_batches_tracked,
                                int32_t set, void* stream) {
    DCV_REQUIRE(m && layer >= 0 && layer < m->L && running_mean_h && running_var_h && num_batches_tracked, "dcv_mlp_bn_state: bad arguments");
    LayerPlan& p = m->layers[layer];
    DCV_REQUIRE(p.bn, "dcv_mlp_bn_state: layer %d has no batch normalisation", layer);
    hipStream_t s = as_stream(stream);
    const size_t bytes = (size_t)p.out * sizeof(float);
    if (set) {
        DCV_CHECK_HIP(hipMemcpyAsync(p.rm, running_mean_h, bytes, hipMemcpyHostToDevice, s));
        DCV_CHECK_HIP(hipMemcpyAsync(p.rv, running_var_h, bytes, hipMemcpyHostToDevice, s));
        p.bn_batches = *num_batches_tracked;
    } else {
        DCV_CHECK_HIP(hipMemcpyAsync(running_mean_h, p.rm, bytes, hipMemcpyDeviceToHost, s));
        DCV_CHECK_HIP(hipMemcpyAsync(running_var_h, p.rv, bytes, hipMemcpyDeviceToHost, s));
        *num_batches_tracked = p.bn_batches;
    }
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    return DCV_OK;
}

extern "C" int dcv_mlp_set_row_sharing(dcv_mlp* m, int32_t enable) {
    DCV_REQUIRE(m, "dcv_mlp_set_row_sharing: null");
    m->no_row_sharing = enable ? 0 : 1;
    return DCV_OK;
}

extern "C" int dcv_mlp_set_lr(dcv_mlp* m, double lr) {
    DCV_REQUIRE(m, "dcv_mlp_set_lr: null");
    m->lr = lr;
    return DCV_OK;
}

extern "C" int dcv_mlp_set_momentum(dcv_mlp* m, double value) {
    DCV_REQUIRE(m, "dcv_mlp_set_momentum: null");
    m->momentum_rt = value;
    return DCV_OK;
}

extern "C" int dcv_mlp_set_upper_grads_callback(dcv_mlp* m, void (*fn)(void*), void* user) {
    DCV_REQUIRE(m, "dcv_mlp_set_upper_grads_callback: null");
    m->upper_cb = fn;
    m->upper_cb_user = user;
    return DCV_OK;
}

extern "C" int dcv_mlp_set_rank(dcv_mlp* m, int32_t rank) {
    DCV_REQUIRE(m && rank >= 0, "dcv_mlp_set_rank: bad arguments");
    m->drop_rank = (uint32_t)rank;
    return DCV_OK;
}

extern "C" int dcv_mlp_layer_output(dcv_mlp* m, int32_t layer, int64_t rows, float* out_d, void* stream) {
    DCV_REQUIRE(m && out_d && layer >= 0 && layer < m->L && rows >= 1 && rows <= m->rows_cap, "dcv_mlp_layer_output: bad arguments");
    if (m->last_path != 0) {
        set_error("dcv_mlp_layer_output: the last forward ran as a fused small-network launch (activations never left LDS); set DCV_NO_SNET=1");
        return DCV_ESTATE;
    }
    const LayerPlan& p = m->layers[layer];
    DCV_CHECK_HIP(hipMemcpy2DAsync(out_d, (size_t)p.out * sizeof(float), p.H, (size_t)p.ldh * sizeof(float), (size_t)p.out * sizeof(float),
                                   (size_t)rows, hipMemcpyDeviceToDevice, as_stream(stream)));
    return DCV_OK;
}

extern "C" int64_t dcv_mlp_dropout_step(const dcv_mlp* m) { return m ? m->drop_step : 0; }
extern "C" int32_t dcv_mlp_last_path(const dcv_mlp* m) { return m ? m->last_path : -1; }
extern "C" int32_t dcv_mlp_last_eval_group(const dcv_mlp* m) { return m ? m->last_eval_group : -1; }
extern "C" int32_t dcv_mlp_last_ride(const dcv_mlp* m) { return m ? m->last_ride : -1; }
extern "C" int32_t dcv_mlp_last_reduce(const dcv_mlp* m) { return m ? m->last_reduce : -1; }
extern "C" float* dcv_mlp_opt_state(dcv_mlp* m, int32_t which) {
    if (!m) return nullptr;
    return which == 0 ? m->adam_m : which == 1 ? m->adam_v : which == 2 ? m->opt_aux : nullptr;
}

extern "C" int dcv_mlp_dropout_mask(dcv_mlp* m, int32_t layer, int64_t step, int64_t rows, float* out_d, void* stream) {
    DCV_REQUIRE(m && out_d && layer >= 0 && layer < m->L && rows >= 1 && step >= 0, "dcv_mlp_dropout_mask: bad arguments");
    const bool keep_mode = m->fwd_train;
    const int64_t keep_step = m->cur_step;
    m->fwd_train = true;
    m->cur_step = step;
    const DropCfg dc = drop_cfg(m, layer);
    m->fwd_train = keep_mode;
    m->cur_step = keep_step;
    const int width = m->layers[layer].out;
    int64_t blocks = cdiv(rows * ((width + 3) / 4), 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), out_d, rows, width, dc);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

extern "C" int dcv_mlp_set_feature_range(dcv_mlp* m, const float* range_h, void* stream) {
    DCV_REQUIRE(m && range_h, "dcv_mlp_set_feature_range: null argument");
    hipStream_t s = as_stream(stream);
    DCV_CHECK_HIP(hipMemcpyAsync(m->feat_range, range_h, m->desc.dims[0] * sizeof(float), hipMemcpyHostToDevice, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    return DCV_OK;
}

extern "C" int dcv_mlp_set_kl_beta(dcv_mlp* m, double beta) {
    DCV_REQUIRE(m && m->vae_d > 0, "dcv_mlp_set_kl_beta: not a variational autoencoder");
    m->kl_beta = beta;
    return DCV_OK;
}

extern "C" int dcv_mlp_set_noise(dcv_mlp* m, const float* eps_d, int64_t rows) {
    DCV_REQUIRE(m && m->vae_d > 0, "dcv_mlp_set_noise: not a variational autoencoder");
    DCV_REQUIRE(rows >= 0 && (eps_d != nullptr || rows == 0), "dcv_mlp_set_noise: bad arguments");
    m->noise = eps_d;
    m->noise_rows = rows;
    m->noise_pos = 0;
    return DCV_OK;
}

extern "C" int64_t dcv_mlp_noise_position(const dcv_mlp* m) { return m ? m->noise_pos : -1; }

extern "C" int dcv_mlp_latent_sample(dcv_mlp* m, int64_t rows, float* out_d, void* stream) {
    DCV_REQUIRE(m && out_d && m->vae_d > 0, "dcv_mlp_latent_sample: bad arguments");
    DCV_REQUIRE(rows >= 1 && rows <= m->last_batch, "dcv_mlp_latent_sample: rows=%lld outside [1, %d]", (long long)rows, m->last_batch);
    if (m->last_path != 0) {
        set_error("dcv_mlp_latent_sample: the last forward ran fused: z never left LDS");
        return DCV_ESTATE;
    }
    DCV_CHECK_HIP(hipMemcpy2DAsync(out_d, (size_t)m->vae_d * sizeof(float), m->vae_z, (size_t)m->ld_z * sizeof(float), (size_t)m->vae_d * sizeof(float),
                                   (size_t)rows, hipMemcpyDeviceToDevice, as_stream(stream)));
    return DCV_OK;
}

extern "C" int dcv_mlp_reset_log(dcv_mlp* m, int32_t capacity, void* stream) {
    DCV_REQUIRE(m && capacity >= 1, "dcv_mlp_reset_log: bad arguments");
    hipStream_t s = as_stream(stream);
    if (capacity > m->log_cap) {
        DCV_CHECK_HIP(hipStreamSynchronize(s));
        if (m->log) (void)hipFree(m->log);
        m->log = nullptr;
        m->log_cap = 0;
        int rc = dmalloc(&m->log, (size_t)capacity * m->log_width);
        if (rc) return rc;
        m->log_cap = capacity;
    }
    DCV_CHECK_HIP(hipMemsetAsync(m->log_count, 0, sizeof(int), s));
    return DCV_OK;
}

extern "C" int dcv_mlp_read_log(dcv_mlp* m, double* out_h, int32_t max_records, int32_t* n_records, void* stream) {
    DCV_REQUIRE(m && out_h && n_records, "dcv_mlp_read_log: null argument");
    hipStream_t s = as_stream(stream);
    int cnt = 0;
    DCV_CHECK_HIP(hipMemcpyAsync(&cnt, m->log_count, sizeof(int), hipMemcpyDeviceToHost, s));
    DCV_CHECK_HIP(hipStreamSynchronize(s));
    if (cnt > m->log_cap) cnt = m->log_cap;
    if (cnt > max_records) cnt = max_records;
    if (cnt > 0) {
        DCV_CHECK_HIP(hipMemcpyAsync(out_h, m->log, (size_t)cnt * m->log_width * sizeof(double), hipMemcpyDeviceToHost, s));
        DCV_CHECK_HIP(hipStreamSynchronize(s));
    }
    *n_records = cnt;
    return DCV_OK;
}

namespace dcv {

static bool act_mask_enabled() {
    static const bool off = env_is("DCV_NO_ACT_MASK", '1');
    return !off;
}

// forward through layers [0, n_run) for `rows` logical rows
// (dropout follows m->fwd_train, which the callers set: training forward on, everything else off)
int run_forward(dcv_mlp* m, const float* Xn, int64_t ld, const RowMap& rows_map, int64_t rows, int n_run, hipStream_t s,
                bool for_backward) {
    for (int l = 0; l < n_run; ++l) {
        LayerPlan& p = m->layers[l];
        p.mask_rows = -1;
        const bool from_z = m->vae_d > 0 && l == m->desc.latent_layer;
        if (from_z) {   // VAE: z = mu + exp(lv / 2) * eps from the heads' output, and the per-block KL partials
            const LayerPlan& hd = m->layers[l - 1];
            m->vae_kblocks = (int)cdiv(rows, kVaeRows);
            hipLaunchKernelGGL(vae_sample_kernel, dim3((unsigned)m->vae_kblocks), dim3(kVaeRows), 0, s, (const float*)hd.H, hd.ldh, rows, m->vae_d,
                               m->eps_cur, m->vae_z, m->ld_z, m->vae_kpart);
            DCV_CHECK_LAUNCH();
        }
        Operand A = l == 0 ? make_operand(Xn, ld, p.in, rows_map)
                           : from_z ? make_operand(m->vae_z, m->ld_z, p.in) : make_operand(layer_out(m, l - 1), m->layers[l - 1].ldh, p.in);
        Operand B = make_operand(m->params + p.w_off, p.in, p.in);
        if (l + 1 < n_run && next_layer_fusable(m, l)) {
            // the narrow Linear behind this layer rides in its epilogue (the whole row of H is in the workgroup)
            LayerPlan& nx = m->layers[l + 1];
            const bool vec = quad_ok(p.H, p.ldh) && quad_ok(m->params + p.b_off, 4) && quad_ok(m->params + nx.w_off, nx.in);
            prof_mark(m, l, 0, 0, s);
            int rc;
            if (nx.out <= 4) {
                EpiBiasActHead<4> epi{p.H, p.ldh, m->params + p.b_off, p.act, vec, m->params + nx.w_off, nx.in, m->params + nx.b_off, nx.out, nx.act, nx.H, nx.ldh};
                epi.drop = drop_cfg(m, l);
                rc = gemm_nt_head4(A, B, rows, p.out, p.in, epi, s, &m->tail);
            } else {
                EpiBiasActHead<8> epi{p.H, p.ldh, m->params + p.b_off, p.act, vec, m->params + nx.w_off, nx.in, m->params + nx.b_off, nx.out, nx.act, nx.H, nx.ldh};
                epi.drop = drop_cfg(m, l);
                rc = gemm_nt_head8(A, B, rows, p.out, p.in, epi, s, &m->tail);
            }
            if (rc) return rc;
            prof_mark(m, l, 0, 1, s);
            prof_mark(m, l + 1, 0, 0, s);
            prof_mark(m, l + 1, 0, 1, s);
            ++l;
            continue;
        }
        EpiBiasAct epi{p.H, p.ldh, m->params + p.b_off, p.act, quad_ok(p.H, p.ldh) && quad_ok(m->params + p.b_off, 4)};
        epi.drop = drop_cfg(m, l);
        if (for_backward && p.mask && act_mask_enabled()) {   // the dgrad of the next layer reads sign(H) instead of H
            epi.mask = p.mask;
            p.mask_rows = rows;
        }
        prof_mark(m, l, 0, 0, s);
        if (p.bn) {   // the derivative of the normalised layer needs the activations themselves, not their signs
            epi.mask = nullptr;
            p.mask_rows = -1;
        }
        int rc = gemm_nt_bias_act(A, B, rows, p.out, p.in, epi, s, &m->tail);
        if (rc) return rc;
        if (p.bn) {
            // training: batch statistics of every forward call of the step -- a Deep-TICA batch is two (x_t rows, then x_lag
            // rows), each normalised by its own statistics and each updating the running ones; evaluation: running statistics
            const bool train = m->fwd_train && for_backward;
            if (train && rows_map.half > 0) {
                rc = bn_forward(m, l, 0, rows_map.half, true, s);
                if (rc == DCV_OK) rc = bn_forward(m, l, rows_map.half, rows - rows_map.half, true, s);
            } else {
                rc = bn_forward(m, l, 0, rows, train, s);
            }
            if (rc) return rc;
        }
        prof_mark(m, l, 0, 1, s);
    }
    return DCV_OK;
}

// Optional (DCV_GRAPH=1; off by default): the launch sequence of a step is captured into a hipGraph each call and the
// instantiated graph of the slot is UPDATED in place (same topology, new kernel arguments: batch offset, Adam bias
// corrections), then launched once.  Needs a capturing-capable (non-null) stream; anything else -- null stream,
// profiling on, first call of a slot, an update the runtime refuses -- takes the plain launches.  Measured on
// MI355X / ROCm 7.2 it buys nothing: the 27 us of gaps per step stay (2.909 vs 2.910 ms at the bench size, 0.454 vs
// 0.449 ms at one eighth of it, and the per-call capture costs the 8192-pair step 3 %), so plain launches are the
// default and the path is kept as a tested option (tests/test_mlp_gpu.py::test_graphed_steps_match_plain_launches).
template <class F>
static int run_graphed(dcv_mlp* m, int slot, hipStream_t s, F&& body) {
    if (!m->graph_on || m->graph_off || s == nullptr || (m->prof_level > 0 && !m->prof_paused) || !m->gwarm[slot]) {
        m->gwarm[slot] = true;
        return body();
    }
    if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        (void)hipGetLastError();
        return body();
    }
    // the host state a replay of body() must not advance twice: step counters, NAdam's mu_product, ASGD's eta, the
    // batch counts of the normalisations (all advanced inside body(): next_opt_args, bn_forward)
    struct HostStep {
        int64_t adam_t, drop_step, cur_step;
        double mu_product, eta;
        int64_t bn_batches[DCV_MAX_LAYERS];
        int64_t noise_pos;        // VAE noise cursor
        const float* eps_cur;
    };
    auto snap = [&]() {
        HostStep h{m->adam_t, m->drop_step, m->cur_step, m->nadam_mu_product, m->asgd_eta, {}, m->noise_pos, m->eps_cur};
        for (int l = 0; l < m->L; ++l) h.bn_batches[l] = m->layers[l].bn_batches;
        return h;
    };
    auto restore = [&](const HostStep& h) {
        m->adam_t = h.adam_t; m->drop_step = h.drop_step; m->cur_step = h.cur_step;
        m->nadam_mu_product = h.mu_product; m->asgd_eta = h.eta;
        for (int l = 0; l < m->L; ++l) m->layers[l].bn_batches = h.bn_batches[l];
        m->noise_pos = h.noise_pos; m->eps_cur = h.eps_cur;
    };
    const HostStep h0 = snap();
    const int rc = body();
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(s, &g);
    if (rc != DCV_OK || ec != hipSuccess || g == nullptr) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        if (rc != DCV_OK) return rc;
        m->gwarm[slot] = false;   // capture failed: run this call (and relearn) without it
        restore(h0);
        return body();
    }
    if (m->gexec[slot]) {
        hipGraphNode_t err_node = nullptr;
        hipGraphExecUpdateResult res = hipGraphExecUpdateSuccess;
        if (hipGraphExecUpdate(m->gexec[slot], g, &err_node, &res) != hipSuccess || res != hipGraphExecUpdateSuccess) {
            (void)hipGetLastError();
            (void)hipGraphExecDestroy(m->gexec[slot]);
            m->gexec[slot] = nullptr;
        }
    }
    if (!m->gexec[slot] && hipGraphInstantiate(&m->gexec[slot], g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        m->gexec[slot] = nullptr;
    }
    (void)hipGraphDestroy(g);
    if (!m->gexec[slot]) {   // nothing was launched yet: replay as plain launches and stop trying on this slot
        m->graph_off = true;
        restore(h0);
        return body();
    }
    DCV_CHECK_HIP(hipGraphLaunch(m->gexec[slot], s));
    m->graph_launches += 1;
    return DCV_OK;
}

// VAE, fused paths: point eps_cur at the next `rows` rows without moving the cursor (moved once the launch went out); false
// when the buffer is too short
bool peek_noise(dcv_mlp* m, int64_t rows) {
    if (m->noise == nullptr || m->noise_pos + rows > m->noise_rows) return false;
    m->eps_cur = m->noise + m->noise_pos * m->vae_d;
    return true;
}
// VAE: the eps rows of the next step (each training / evaluation step consumes `batch` rows of the noise buffer); checked
// before anything is launched
static int take_noise(dcv_mlp* m, int64_t batch) {
    if (!peek_noise(m, batch)) {
        set_error("dcv_mlp step: the VAE noise buffer holds %lld rows, %lld used, a step of %lld rows needs more (dcv_mlp_set_noise)",
                  (long long)m->noise_rows, (long long)m->noise_pos, (long long)batch);
        return DCV_ESTATE;
    }
    m->noise_pos += batch;
    return DCV_OK;
}

// fuse_head: 0 = statistics only (a data-parallel caller all-reduces them before dcv_mlp_backward); 1 / 2 = one-GPU
// training / evaluation step: the last block of the statistics launch also runs the loss head (batch = global batch)
int forward_impl(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t train, void* stream,
                 int fuse_head) {
    DCV_REQUIRE(m && Xn_d, "dcv_mlp_forward: null argument");
    DCV_REQUIRE(batch >= 1 && batch <= m->desc.max_batch, "dcv_mlp_forward: batch=%d exceeds max_batch=%d", batch, m->desc.max_batch);
    DCV_REQUIRE(ld >= m->desc.dims[0], "dcv_mlp_forward: ld=%lld < F=%d", (long long)ld, m->desc.dims[0]);
    if (fuse_head) DCV_REQUIRE(m->log && m->log_cap > 0, "dcv_mlp step: call dcv_mlp_reset_log first");
    // torch.nn.BatchNorm1d raises on a training forward call of one row ("Expected more than 1 value per channel when training");
    // every forward call of a step -- the batch, or each half of a Deep-TICA batch -- has `batch` rows
    DCV_REQUIRE(!(train && m->any_bn && batch == 1), "dcv_mlp_forward: a training forward of one row per call through a batch normalisation");
    if (m->vae_d > 0) {   // after every argument check, before any state changes: a refused step leaves the engine as it was
        const int rcn = take_noise(m, batch);
        if (rcn) return rcn;
    }
    g_launch_ev = LaunchEvents{};   // an offer left behind by a launch that failed half way
    step_begin(m, train != 0);
    step_done(m, 0, m->last_batch, false);   // (a forward that fails below leaves no batch behind)
    hipStream_t s = as_stream(stream);
    if (m->desc.model == DCV_MODEL_DEEPTICA && !(m->snet_dt_tried && m->snet_dt == nullptr)) {
        // a network that fits in LDS: forward, batch statistics and (one-GPU steps) the loss head in ONE launch (snet_dt.hip)
        prof_mark(m, 0, 0, 0, s);
        // the loss head runs inside the forward launch only when no backward follows (evaluation step); a training step's
        // head is evaluated by the backward launch's workgroups beside their staging (snet_dt.hip)
        const int rcs = snet_dt_forward(m, Xn_d, ld, idx_d, row0, batch, fuse_head == 2 ? 2 : 0, fuse_head != 2, s);
        if (rcs < 0) return rcs;
        if (rcs == DCV_OK) {
            prof_mark(m, 0, 0, 1, s);
            step_done(m, 2, batch, fuse_head == 2);   // (a training step's forward left its blob for the backward)
            return DCV_OK;
        }
        if (prof_on(m, 0)) g_launch_ev = LaunchEvents{};   // not applicable: the layer-by-layer path marks its own launches
    }
    const RowMap rm = batch_rows(m, idx_d, row0, batch);
    const int64_t R = rows_of(m, idx_d, batch);
    int rc = run_forward(m, Xn_d, ld, rm, R, m->L, s, fuse_head != 2);   // the one-GPU evaluation step has no backward: no sign masks
    if (rc) return rc;
    const LayerPlan& last = m->layers[m->L - 1];
    const float* net_out = layer_out(m, m->L - 1);   // the network's output: behind the last layer's normalisation when it has one
    bool head_ran = fuse_head != 0;
    if (m->desc.model == DCV_MODEL_DEEPTICA) rc = tica_stats(m, net_out, last.ldh, batch, lag_offset(m, idx_d, batch), fuse_head, &head_ran, s);
    else rc = ae_sse(m, net_out, last.ldh, Xn_d, ld, rm, R, batch, fuse_head != 0, s);
    if (rc) return rc;
    step_done(m, 0, batch, head_ran);
    return DCV_OK;
}

// ------------------------------------------------------------------ backward, layer by layer
// what the parts of one pass share: dz_cur holds dL/dz of the layer in turn, a part that hands a gradient down writes dz_nxt
// and swaps; bblocks = bias-gradient partials the layer in turn finds in its bpart; ra collects what the reduction folds
struct Backward {
    dcv_mlp* m;
    const float* Xn;   // the caller's features, their row stride, the batch's index list (or null)
    int64_t ld;
    const int64_t* idx;
    RowMap rm;         // the batch's rows and their count R (batch_rows, rows_of)
    int64_t R;
    int32_t batch;
    int64_t global_batch;
    hipStream_t s;
    float *dz_cur, *dz_nxt;
    int bblocks;
    ReduceArgs ra;
    bool fuse_opt = false;   // one-GPU training step: the update rides in the reduction
    bool ridden = false;     // ride_upper took everything but the weights of layer 0, with the update arguments `oa`
    OptArgs oa{};
};

// Deep-TICA after a fused forward (snet_dt.hip): one backward launch from its blob, then the reduction (+ optimiser)
static int backward_blob(dcv_mlp* m, int32_t batch, int64_t global_batch, bool head_in_bwd, bool fuse_opt, hipStream_t s) {
    if (!m->snet_fwd_valid) {
        set_error("dcv_mlp_backward: the fused forward of this batch kept no activations (evaluation step)");
        return DCV_ESTATE;
    }
    ReduceArgsView v;
    prof_mark(m, 0, 1, 0, s);
    const int rc = snet_dt_backward(m, batch, global_batch, head_in_bwd, &v, s);
    if (rc) return rc;
    prof_mark(m, 0, 1, 1, s);
    return finish_grads(m, reduce_args_of(m, v), fuse_opt, false, s);
}
// dL/dz of the last layer -> dz_cur, and its bias-gradient partials.  fused_head: head_backward_layer does both instead.
static int seed_gradient(Backward& c, bool fused_head) {
    dcv_mlp* m = c.m;
    const LayerPlan& last = m->layers[m->L - 1];
    // a normalised last layer: the loss gradient is taken w.r.t. the normalised output; activation derivative and dropout
    // of the Linear underneath are applied by the normalisation's backward pass
    const float* net_out = layer_out(m, m->L - 1);
    const int act = last.bn ? DCV_ACT_NONE : last.act;
    const DropCfg drop = last.bn ? kNoDrop : drop_cfg(m, m->L - 1);
    const float hscale = last.bn ? 1.f : drop_hscale(m, m->L - 1);
    int rc = DCV_OK;
    if (!fused_head)
        rc = loss_gradient(m, net_out, last.ldh, c.Xn, c.ld, c.rm, c.R, c.batch, lag_offset(m, c.idx, c.batch), c.global_batch, act, c.dz_cur, drop, hscale, c.s);
    // bias-gradient partials of the last layer come from a column-sum pass over dZ_last; those of
    // every other layer fall out of the dgrad epilogue that produces its dZ
    c.bblocks = (int)cdiv(c.R, kColsumRows);
    if (rc == DCV_OK && !fused_head && !last.bn) {
        hipLaunchKernelGGL(colsum_kernel, dim3(c.bblocks), dim3(256), 0, c.s, c.dz_cur, c.R, last.out, m->ld_dz, last.bpart);
        DCV_CHECK_LAUNCH();
    }
    return rc;
}
// dz_cur holds dL/d(normalised output) of layer l: back through the normalisation, the dropout and the activation of the
// layer, in place; its passes also leave the gradient partials of the normalisation's weight / bias and the bias-gradient
// partials of this Linear
static int norm_backward(Backward& c, int l) {
    const LayerPlan& p = c.m->layers[l];
    const bool two = c.rm.half > 0;   // two forward calls (x_t rows, x_lag rows), each with its own statistics
    int nb = 0;
    const int rc = bn_backward(c.m, l, c.dz_cur, c.m->ld_dz, two ? 2 : 1, two ? (int64_t)c.rm.half : c.R, p.act, drop_hscale(c.m, l), drop_cfg(c.m, l), &nb, c.s);
    if (rc) return rc;
    c.bblocks = nb;
    c.ra.l[c.m->L + l] = ReduceDesc{p.bn_gpart, p.bn_bpart, p.g_off, p.be_off, p.out, p.out, nb, nb, 0, 0};   // weight / bias of the normalisation
    return DCV_OK;
}
// loss gradient, both bias gradients, wgrad and dgrad of the narrow last layer in one pass over H_{L-2}
static int head_backward_layer(Backward& c) {
    dcv_mlp* m = c.m;
    const int l = m->L - 1;
    prof_mark(m, l, 1, 0, c.s);
    const int rc = head_backward(m, c.R, c.batch, lag_offset(m, c.idx, c.batch), c.dz_nxt, &c.bblocks, c.s);
    if (rc) return rc;
    prof_mark(m, l, 1, 1, c.s);
    prof_mark(m, l, 2, 0, c.s);
    prof_mark(m, l, 2, 1, c.s);
    c.ra.l[l] = linear_reduce_desc(m->layers[l], c.bblocks, c.bblocks);
    std::swap(c.dz_cur, c.dz_nxt);
    return DCV_OK;
}
// the weight-gradient split of layer l over this pass's rows: noted for the reduction; returns the rows per chunk
static int64_t plan_wgrad(Backward& c, int l) {
    const LayerPlan& p = c.m->layers[l];
    int64_t kc, splits;
    wgrad_plan(p.out, p.in, c.R, &kc, &splits);
    if (splits > p.max_splits) {
        splits = p.max_splits;
        kc = cdiv(cdiv(c.R, splits), 32) * 32;
        splits = cdiv(c.R, kc);
    }
    c.ra.l[l] = linear_reduce_desc(p, (int)splits, c.bblocks);
    return kc;
}
static EpiSlab slab_epi(const LayerPlan& p) { return EpiSlab{p.slab, p.out, p.in, 1, 0, quad_ok(p.slab, p.in), p.max_splits}; }
// wgrad of layer l as a launch of its own: dW = dZ^T In  (M = out, N = in, K = rows), In = the rows behind B
static int wgrad_alone(Backward& c, int l, const Operand& B, int64_t kc) {
    const LayerPlan& p = c.m->layers[l];
    prof_mark(c.m, l, 1, 0, c.s);
    const int rc = gemm_tn_slab(make_operand(c.dz_cur, c.m->ld_dz, p.out), B, p.out, p.in, c.R, kc, slab_epi(p), c.s);
    if (rc) return rc;
    prof_mark(c.m, l, 1, 1, c.s);
    return DCV_OK;
}
// VAE, first decoder Linear: wgrad against z; dgrad dL/dz (no activation between the heads and z), turned in
// place into [dL/dmu | dL/dlv] by the reparameterisation's backward; the heads' bias partials by a column sum
static int latent_backward_layer(Backward& c, int l) {
    dcv_mlp* m = c.m;
    const LayerPlan& p = m->layers[l];
    const LayerPlan& hd = m->layers[l - 1];
    const int64_t kc = plan_wgrad(c, l);
    int rc = wgrad_alone(c, l, make_operand(m->vae_z, m->ld_z, p.in), kc);
    if (rc) return rc;
    Operand A = make_operand(c.dz_cur, m->ld_dz, p.out);
    Operand Bd = make_operand(m->params + p.w_off, p.in, p.in);
    EpiActGrad eg{c.dz_nxt, m->ld_dz, m->vae_z, m->ld_z, DCV_ACT_NONE, hd.bpart, p.in, quad_ok(c.dz_nxt, m->ld_dz) && quad_ok(m->vae_z, m->ld_z)};
    int dblocks = 0;
    prof_mark(m, l, 2, 0, c.s);
    rc = gemm_nn_act_grad(A, Bd, c.R, p.in, p.out, eg, c.s, &dblocks, &m->tail);
    if (rc) return rc;
    hipLaunchKernelGGL(vae_sample_backward_kernel, dim3((unsigned)cdiv(c.R, kVaeRows)), dim3(kVaeRows), 0, c.s, (const float*)hd.H, hd.ldh, c.R, m->vae_d,
                       m->eps_cur, c.dz_nxt, m->ld_dz, (float)(m->kl_beta / (double)c.global_batch));
    DCV_CHECK_LAUNCH();
    c.bblocks = (int)cdiv(c.R, kColsumRows);
    hipLaunchKernelGGL(colsum_kernel, dim3(c.bblocks), dim3(256), 0, c.s, (const float*)c.dz_nxt, c.R, hd.out, m->ld_dz, hd.bpart);
    DCV_CHECK_LAUNCH();
    prof_mark(m, l, 2, 1, c.s);
    std::swap(c.dz_cur, c.dz_nxt);
    return DCV_OK;
}
// the generic layer: wgrad, and above layer 0 the dgrad  dZ_prev = (dZ W) * act'(H_prev)   (M = rows, N = in, K = out)
static int backward_layer(Backward& c, int l) {
    dcv_mlp* m = c.m;
    hipStream_t s = c.s;
    const LayerPlan& p = m->layers[l];
    const int64_t R = c.R;
    const int64_t kc = plan_wgrad(c, l);
    if (l == 0) {
        const Operand X = make_operand(c.Xn, c.ld, p.in, c.rm);
        if (c.fuse_opt) {
            // the gradients that do not wait for this product reduce and update inside its launch (mlp_opt.hip: ride_upper); a
            // stamped launch stays one stamped launch, its interval now includes the ride-along blocks
            prof_mark(m, l, 1, 0, s);
            const int rc = ride_upper(m, c.ra, make_operand(c.dz_cur, m->ld_dz, p.out), X, p.out, p.in, R, kc, slab_epi(p), &c.oa, s);
            if (rc < 0) return rc;
            if (rc == DCV_OK) {
                prof_mark(m, l, 1, 1, s);
                c.ridden = true;
                return DCV_OK;
            }
        }
        return wgrad_alone(c, l, X, kc);
    }
    const LayerPlan& q = m->layers[l - 1];
    Operand A = make_operand(c.dz_cur, m->ld_dz, p.out);
    Operand B = make_operand(layer_out(m, l - 1), q.ldh, p.in);
    const EpiSlab epi = slab_epi(p);
    Operand Bd = make_operand(m->params + p.w_off, p.in, p.in);
    EpiActGrad eg{c.dz_nxt, m->ld_dz, q.H, q.ldh, q.act, q.bpart, q.out, quad_ok(c.dz_nxt, m->ld_dz) && quad_ok(q.H, q.ldh)};
    if (q.mask && q.mask_rows == R) {   // written by this step's forward with the same (rows, width) => same tiling
        eg.mask = q.mask;
        eg.slope = q.act == DCV_ACT_LEAKY_RELU ? 0.01f : 0.f;
    }
    eg.drop = drop_cfg(m, l - 1);
    eg.hscale = drop_hscale(m, l - 1);
    if (q.bn) {   // a normalised layer below: hand down the raw product dL/d(its normalised output); bn_backward does the rest
        eg.act = DCV_ACT_NONE;
        eg.mask = nullptr;
        eg.drop = kNoDrop;
        eg.hscale = 1.f;
    }
    // the two products read the same dZ and neither reads the other's output: one launch when the pair form applies
    prof_mark(m, l, 1, 0, s);
    prof_mark(m, l, 2, 0, s);
    int rc = launch_wgrad_dgrad(A, B, p.out, p.in, R, kc, epi, A, Bd, R, p.in, p.out, eg, &c.bblocks, &m->tail, s);
    if (rc < 0) return rc;
    if (rc == 1) {
        rc = gemm_tn_slab(A, B, p.out, p.in, R, kc, epi, s);
        if (rc) return rc;
        prof_mark(m, l, 1, 1, s);
        prof_mark(m, l, 2, 0, s);
        rc = gemm_nn_act_grad(A, Bd, R, p.in, p.out, eg, s, &c.bblocks, &m->tail);
        if (rc) return rc;
        prof_mark(m, l, 2, 1, s);
    } else {
        prof_mark(m, l, 1, 1, s);
        prof_mark(m, l, 2, 1, s);
    }
    std::swap(c.dz_cur, c.dz_nxt);
    return DCV_OK;
}

int backward_impl(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int64_t global_batch, int32_t train,
                  void* stream, bool fuse_opt) {
    DCV_REQUIRE(m && Xn_d, "dcv_mlp_backward: null argument");
    g_launch_ev = LaunchEvents{};
    if (m->last_batch != batch) {
        set_error("dcv_mlp_backward: batch=%d does not match the preceding forward (%d)", batch, m->last_batch);
        return DCV_ESTATE;
    }
    DCV_REQUIRE(global_batch >= batch, "dcv_mlp_backward: global_batch=%lld < batch=%d", (long long)global_batch, batch);
    if (m->any_drop && train && !m->fwd_train) {
        set_error("dcv_mlp_backward: train=1 after an evaluation-mode forward (dropout masks would not match)");
        return DCV_ESTATE;
    }
    DCV_REQUIRE(m->log && m->log_cap > 0, "dcv_mlp_backward: call dcv_mlp_reset_log first");
    hipStream_t s = as_stream(stream);
    const bool tica = m->desc.model == DCV_MODEL_DEEPTICA;
    const bool head_in_bwd = tica && m->last_path == 2 && train && !m->head_done && m->snet_fwd_valid;   // the fused backward evaluates the head itself
    int rc = loss_record(m, global_batch, train != 0, head_in_bwd, s);
    if (rc || !train) return rc;
    m->last_ride = 0;
    if (tica && m->last_path == 2) return backward_blob(m, batch, global_batch, head_in_bwd, fuse_opt, s);
    const int L = m->L;
    Backward c{m, Xn_d, ld, idx_d, batch_rows(m, idx_d, row0, batch), rows_of(m, idx_d, batch), batch, global_batch, s, m->dZ[0], m->dZ[1], 0, ReduceArgs{}};
    c.ra.L = L;
    c.fuse_opt = fuse_opt;
    const bool fused_head = tica && head_fusable(m);
    rc = seed_gradient(c, fused_head);
    bool upper_done = false;
    for (int l = L - 1; l >= 0 && rc == DCV_OK; --l) {
        // Data-parallel overlap: everything the gradients of layers 1 .. L-1 need has been enqueued (their slabs, and
        // the bias partials of every layer).  Reduce them now and tell the caller, who starts their all-reduce on a
        // side stream while the largest product of the step -- the layer-0 weight gradient -- still runs here.
        if (l == 0) rc = reduce_upper(m, c.ra, fuse_opt, &upper_done, s);
        if (rc == DCV_OK && m->layers[l].bn) rc = norm_backward(c, l);
        if (rc) break;
        if (fused_head && l == L - 1) rc = head_backward_layer(c);
        else if (m->vae_d > 0 && l == m->desc.latent_layer) rc = latent_backward_layer(c, l);
        else rc = backward_layer(c, l);
    }
    if (rc) return rc;
    return finish_grads(m, c.ra, fuse_opt, upper_done, s, c.ridden ? &c.oa : nullptr);
}

// One-GPU autoencoder step as ONE fused launch (+ the gradient reduction with the optimiser update) when the network
// fits in LDS (snet.hip); 1 = not applicable: the caller runs the layer-by-layer path.
static int snet_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t train, void* stream) {
    if ((m->desc.model != DCV_MODEL_AE && m->desc.model != DCV_MODEL_VAE) || m->any_drop || m->any_bn || (m->snet_tried && m->snet == nullptr)) return 1;
    if (!(Xn_d && batch >= 1 && batch <= m->desc.max_batch && ld >= m->desc.dims[0] && m->log && m->log_cap > 0)) return 1;   // the general path reports it
    if (m->vae_d > 0 && !peek_noise(m, batch)) return 1;   // the general path refuses it
    hipStream_t s = as_stream(stream);
    ReduceArgsView v;
    prof_mark(m, 0, 0, 0, s);   // profiling: the fused launch is reported under both layer-0 classes (forward, weight gradient)
    prof_mark(m, 0, 1, 0, s);
    int rc = snet_ae_step(m, Xn_d, ld, RowMap{idx_d, row0, 0, 0}, batch, batch, train, &v, s);
    if (rc) return rc;
    if (m->vae_d > 0) m->noise_pos += batch;   // the launch took the rows peek_noise pointed at
    prof_mark(m, 0, 0, 1, s);
    prof_mark(m, 0, 1, 1, s);
    step_begin(m, train != 0);
    step_done(m, 1, batch, false);
    if (!train) return DCV_OK;
    return finish_grads(m, reduce_args_of(m, v), true, false, s);
}

}  // namespace dcv

extern "C" int dcv_mlp_profile_begin(dcv_mlp* m, int32_t max_steps, int32_t level) {
    DCV_REQUIRE(m && max_steps >= 1 && (level == 1 || level == 2), "dcv_mlp_profile_begin: bad arguments");
    const size_t need = (size_t)3 * m->L * max_steps * 2;
    while (m->prof_ev.size() < need) {
        hipEvent_t e;
        DCV_CHECK_HIP(hipEventCreate(&e));
        m->prof_ev.push_back(e);
    }
    m->prof_cap = max_steps;
    m->prof_cnt.assign((size_t)3 * m->L, 0);
    m->prof_kind_off = 0;
    m->prof_paused = false;
    m->prof_level = level;
    return DCV_OK;
}

extern "C" int dcv_mlp_profile_pause(dcv_mlp* m, int32_t paused) {
    DCV_REQUIRE(m, "dcv_mlp_profile_pause: null");
    m->prof_paused = (paused & 1) != 0;
    m->prof_kind_off = (paused >> 1) & 7;   // bit 1 / 2 / 3: forward / weight-gradient / input-gradient launches carry no events
    return DCV_OK;
}

extern "C" int dcv_mlp_profile_end(dcv_mlp* m, double* ms_h, int32_t* counts_h) {
    DCV_REQUIRE(m && ms_h && counts_h, "dcv_mlp_profile_end: null argument");
    const int level = m->prof_level;
    m->prof_level = 0;
    for (int c = 0; c < 3 * m->L; ++c) {
        ms_h[c] = 0.0;
        counts_h[c] = 0;
        const int layer = c / 3, kind = c % 3;
        if (level < 2 && layer != 0) continue;
        if (kind == 2 && layer == 0) continue;  // the first layer has no dgrad
        const int steps = (size_t)c < m->prof_cnt.size() ? m->prof_cnt[c] : 0;
        for (int i = 0; i < steps; ++i) {
            hipEvent_t a = m->prof_ev[((size_t)c * m->prof_cap + i) * 2 + 0];
            hipEvent_t b = m->prof_ev[((size_t)c * m->prof_cap + i) * 2 + 1];
            DCV_CHECK_HIP(hipEventSynchronize(b));
            float ms = 0.f;
            DCV_CHECK_HIP(hipEventElapsedTime(&ms, a, b));
            ms_h[c] += (double)ms;
            counts_h[c] += 1;
        }
    }
    return DCV_OK;
}

extern "C" int dcv_mlp_forward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                               int32_t train, void* stream) {
    DCV_REQUIRE(m, "dcv_mlp_forward: null");
    return run_graphed(m, 1, as_stream(stream), [&] { return forward_impl(m, Xn_d, ld, idx_d, row0, batch, train, stream); });
}

extern "C" int dcv_mlp_backward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                                int64_t global_batch, int32_t train, void* stream) {
    DCV_REQUIRE(m, "dcv_mlp_backward: null");
    if (!train) return backward_impl(m, Xn_d, ld, idx_d, row0, batch, global_batch, train, stream);   // one tiny launch
    return run_graphed(m, 2, as_stream(stream), [&] { return backward_impl(m, Xn_d, ld, idx_d, row0, batch, global_batch, train, stream); });
}

extern "C" int dcv_mlp_apply(dcv_mlp* m, void* stream) { return apply_impl(m, stream); }
extern "C" int64_t dcv_mlp_graph_launches(const dcv_mlp* m) { return m ? m->graph_launches : 0; }
extern "C" int dcv_mlp_set_graph(dcv_mlp* m, int32_t enable) {
    DCV_REQUIRE(m, "dcv_mlp_set_graph: null");
    m->graph_on = enable != 0;
    return DCV_OK;
}

// a one-GPU step: the fused small-network launch when it applies, else forward (with the loss head) and backward -- for a
// training step with the reduction + optimiser update in one launch
static int one_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t train, void* stream) {
    int rc = snet_step(m, Xn_d, ld, idx_d, row0, batch, train, stream);
    if (rc != 1) return rc;
    rc = forward_impl(m, Xn_d, ld, idx_d, row0, batch, train, stream, train ? 1 : 2);
    if (rc) return rc;
    return backward_impl(m, Xn_d, ld, idx_d, row0, batch, batch, train, stream, train != 0);
}
extern "C" int dcv_mlp_train_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                                  void* stream) {
    DCV_REQUIRE(m, "dcv_mlp_train_step: null");
    return run_graphed(m, 0, as_stream(stream), [&] { return one_step(m, Xn_d, ld, idx_d, row0, batch, 1, stream); });
}

extern "C" int dcv_mlp_eval_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                                 void* stream) {
    DCV_REQUIRE(m, "dcv_mlp_eval_step: null");
    return run_graphed(m, 3, as_stream(stream), [&] { return one_step(m, Xn_d, ld, idx_d, row0, batch, 0, stream); });
}

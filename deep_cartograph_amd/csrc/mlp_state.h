// State of the MLP engine (dcv_mlp) and what the translation units that implement it share: mlp.hip (core), mlp_opt.hip,
// mlp_heads.hip, mlp_passes.hip, bn.hip, snet.hip, snet_dt.hip.
#pragma once
#include "gemm_kernels.h"
#include <stdlib.h>
#include <vector>

namespace dcv {

constexpr int kMaxTicaDim = 16;

// Workspace of a grouped validation pass of the block engine (mlp_passes.hip: eval_group): ONE device allocation, held by the engine
// from the first grouped pass on and grown only when a later pass wants more members or longer batches than it holds.
struct EvalGroupWs {
    char* base = nullptr;
    size_t bytes = 0;
    int members = 0, batch = 0;   // the layout it is carved into (eval_group_layout): members, pairs per batch, rows per member
    int64_t rows = 0;
    bool failed = false;       // an allocation failed once: the engine keeps stepping batch by batch
};

struct LayerPlan {   // (value-initialised by the engine: every member starts as zero / null unless it says otherwise)
    int in, out, act;
    int64_t w_off, b_off;      // offsets into the flat parameter buffer (floats, 16-byte aligned)
    int64_t ldh;               // row stride of the activation buffer
    float* H;                  // [rows][ldh] post-activation output
    // wgrad split-K
    int64_t k_chunk_cap;       // rows per split at full capacity
    int64_t max_splits;
    float* slab;               // [max_splits][out][in]
    float* bpart;              // [bias_blocks_cap][out]
    unsigned long long* mask;  // sign mask of H in the forward epilogue's thread layout (ReLU family), or null
    int64_t mask_rows = -1;    // row count of the training forward that wrote it (-1: stale)
    // batch normalisation behind this Linear (bn.hip), or bn == 0
    int bn;
    int64_t g_off = -1, be_off = -1;   // weight / bias of the normalisation in the flat parameter buffer (-1 without one)
    float* Y;                  // [rows][ldh] normalised output (input of the next layer); H keeps the values it was computed from
    float *rm, *rv;            // running mean / variance [out]
    double* bn_stat;           // [2 forward calls][mean | invstd][out] of the last training forward
    double* bn_part;           // statistics partials [blocks][2][out]
    float *bn_gpart, *bn_bpart;   // gradient partials of weight / bias [blocks][out]
    int64_t bn_batches;        // num_batches_tracked
};

}  // namespace dcv

struct dcv_mlp {   // created value-initialised (dcv_mlp_create): every member starts as zero / null / false
    dcv_mlp_desc desc;
    int L;
    int d_out;                 // dims[L]
    int64_t rows_cap;          // rows per step at max_batch
    int64_t n_params;
    std::vector<dcv::LayerPlan> layers;
    float *params, *grads, *adam_m, *adam_v;
    float* opt_aux;            // third optimiser state (amsgrad maximum / centred RMSprop gradient average) or null
    double momentum_rt;        // beta1 (Adam family) or momentum (SGD, RMSprop): dcv_mlp_set_momentum
    double nadam_mu_product;   // NAdam: the float32 state mu_product, as torch reads it back
    double asgd_eta;           // ASGD: the float32 state eta
    bool any_drop;             // some layer has dropout p > 0
    bool any_bn;               // some layer is followed by a batch normalisation
    bool fwd_train;            // the last forward ran in training mode (dropout active): backward must agree
    dcv::TailWs tail;          // workspace of the contraction-split tail tile of row-tiled products (gemm.h: GemmDims::tail_split)
    dcv::EvalGroupWs eval_ws;  // grouped validation pass (dcv_mlp_eval_steps, block engine)
    int last_eval_group;       // members of the first grouped launch of the last dcv_mlp_eval_steps call (0: it stepped batch by batch)
    int last_ride;             // reduction blocks that rode in the layer-0 weight-gradient launch of the last backward (0: none; ride_upper)
    int last_reduce;           // kernel of the final reduction of the last backward: 0 none yet, 1 flat-grid quad, 2 4-wave, 3 16-wave (launch_reduce)
    void (*upper_cb)(void*);   // data-parallel overlap hook (dcv_mlp_set_upper_grads_callback) or null
    void* upper_cb_user;
    bool head_done;            // the last forward already ran the d x d loss head inside its statistics launch (one-GPU steps)
    int64_t drop_step;         // training forwards so far = step field of the next forward's dropout counters
    int64_t cur_step;          // step field of the last training forward
    uint32_t drop_rank;        // mixed into the key of the dropout counters (dcv_mlp_set_rank): the ranks of a data-parallel run draw independent masks
    void* snet;                // plan of the fused small-network step (snet.hip) or null
                               //   (snet / snet_dt are set while their plan is still being built, so that a failed build is released by
                               //   snet_free / snet_dt_free: non-null does not mean complete until snet_build / snet_dt_build have returned)
    bool snet_tried;           // the plan was attempted once (null afterwards = not applicable)
    float* snet_img;           // zero-padded LDS image of every weight / bias of the fused small-network kernels, kept current by the
    int* snet_img_idx;         //   optimiser (img[img_idx[i]] mirrors params[i]; -1: not part of the image); null until a plan builds it
    int snet_img_floats;
    void* snet_dt;             // plan of the fused small-network Deep-TICA forward / backward (snet_dt.hip) or null
    bool snet_dt_tried;
    bool snet_fwd_valid;       // the last forward went through snet_dt_forward and left its blob for the backward
    int last_path;             // path of the last step / forward: 0 layer by layer, 1 fused autoencoder step, 2 fused Deep-TICA kernels
    float* dZ[2];
    int64_t ld_dz;
    double* stats;             // device
    int stats_len;
    double* gradp;             // Deep-TICA: [mu d | Gu d*d | Gv d*d | c d], float64 (see tica_dF_kernel)
    double* spart;             // stats partials
    int spart_blocks;
    double* log;
    int* log_count;
    unsigned* ticket;          // block counter of the single-launch statistics reduction (zero between launches)
    hipGraphExec_t gexec[4];   // instantiated step graphs (train step, forward, backward, eval step) or null
    bool gwarm[4];             // the slot ran once outside capture (lazy module loading, first-use attributes)
    bool graph_on;             // step graphs requested (dcv_mlp_set_graph; default from DCV_GRAPH=1)
    bool graph_off;            // graph instantiation failed once: plain launches from then on
    int64_t graph_launches;    // steps / half-steps that went out as one graph launch
    bool prof_paused;          // profiling armed but skipped for the current calls (dcv_mlp_profile_pause)
    int log_cap, log_width;
    float* feat_range;         // AE, VAE
    // VAE (DCV_MODEL_VAE): Linear latent_layer - 1 is the two heads [mean | log-variance] (2 * vae_d columns), Linear
    // latent_layer reads z = mean + exp(log-variance / 2) * eps
    int vae_d;                 // latent dimension d (0: not a VAE)
    float* vae_z;              // [rows_cap][ld_z] sampled latent of the last forward
    int64_t ld_z;
    double* vae_kpart;         // per-block KL partials of the sampling kernel
    int vae_kblocks;           // blocks of the last sampling launch
    double kl_beta;            // weight of the KL term (dcv_mlp_set_kl_beta)
    const float* noise;        // caller's eps buffer [noise_rows][vae_d] (dcv_mlp_set_noise) or null
    int64_t noise_rows, noise_pos;
    const float* eps_cur;      // eps rows of the last forward (noise + its first row * vae_d)
    float *ident, *zeros_d, *ones_d;  // helpers for inference
    float* proj_ws;
    size_t proj_ws_bytes;
    int64_t adam_t;
    double lr;
    // bookkeeping of the last forward (backward must match)
    int32_t last_batch;
    int no_row_sharing;        // diagnostic: evaluate contiguous Deep-TICA batches as two separate halves
    // optional per-kernel timing with HIP events on the launch stream (bench.py roofline)
    int prof_level, prof_cap;
    int prof_kind_off;                // kinds (bit 0 fwd, 1 wgrad, 2 dgrad) whose launches are not sampled right now
    std::vector<int> prof_cnt;        // samples taken per class
    std::vector<hipEvent_t> prof_ev;  // [class][step][2], class = 3*layer + {0 fwd, 1 wgrad, 2 dgrad}
};


namespace dcv {
// gradient partials of a fused small-network step, as the split-K reduction wants them (per layer: [splits][out * in] and
// [bblocks][out])
struct ReduceArgsView {
    const float* slab[DCV_MAX_LAYERS];
    const float* bpart[DCV_MAX_LAYERS];
    int splits[DCV_MAX_LAYERS];
    int bblocks[DCV_MAX_LAYERS];
    int64_t wstride[DCV_MAX_LAYERS], bstride[DCV_MAX_LAYERS];   // floats between consecutive partials (multiples of 4)
};
// a batched validation pass (dcv_mlp_eval_steps) of a fused small-network engine: at most this many batches / workgroups per launch
// (the plans allocate their per-batch tickets and per-workgroup partials for these bounds when they are built: no allocation
// lands in a timed validation pass)
constexpr int kEvalBatchesPerLaunch = 64;
// The block engine's grouped pass keeps one segment of every layer's output per member, plus the member's tail workspace and
// statistics partials: as many members as fit this budget.  The headline network (512-256-128-4, batches of 8192 pairs = 8202
// shared rows) needs 8202 rows x (256 + 128 + 4) floats = 12.7 MB of activations + 2 MB of tail workspace per member:
// 18 members (16 would be 204 MB of activations).  Measured on that shape: 8 members 21.6 us per batch, 18 members 19.3.
constexpr size_t kEvalGroupBudgetBytes = 256ull << 20;
constexpr int64_t kEvalWorkgroupsPerLaunch = 4096;
// snet.hip: the whole autoencoder step in one launch when the network fits in LDS; 1 = not applicable
// R rows of this rank, `batch` = the GLOBAL batch (loss scale 2 / (batch * F)); write_log = false: the caller logs (after an all-reduce)
int snet_ae_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const RowMap& rm, int64_t R, int64_t batch, int train, ReduceArgsView* ra,
                 hipStream_t s, bool write_log = true, int nb = 1);   // nb > 1: that many evaluation batches of R rows in one launch
int snet_ae_tile_rows(dcv_mlp* m, int64_t R = 0);   // rows per workgroup of the fused kernel for batches of R rows (builds the plan on first use); 0: not applicable
void snet_free(dcv_mlp* m);
int snet_ae_last_tile_rows(const dcv_mlp* m);   // rows per workgroup of the last fused autoencoder launch (0: none yet)
// the weight image both fused small-network plans stage from (snet.hip); repack: after the parameters were written by anyone
// but the optimiser (dcv_mlp_set_params)
bool snet_image_build(dcv_mlp* m);
int snet_image_repack(dcv_mlp* m, hipStream_t s);
void snet_image_free(dcv_mlp* m);
// snet_dt.hip: Deep-TICA forward (+ statistics, + loss head) and backward of a network that fits in LDS; 1 = not applicable
// nb > 1 (head == 2, no blob): that many evaluation batches of `batch` pairs in one launch, batch j = the pairs [j * batch, (j + 1) * batch)
int snet_dt_forward(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int head, bool keep_blob,
                    hipStream_t s, int nb = 1);
int snet_dt_backward(dcv_mlp* m, int32_t batch, int64_t global_batch, bool head, ReduceArgsView* ra, hipStream_t s);
void snet_dt_free(dcv_mlp* m);
int snet_dt_last_tile_rows(const dcv_mlp* m);   // rows per workgroup of the last fused Deep-TICA forward (0: none yet)
// bn.hip
int bn_forward(dcv_mlp* m, int l, int64_t row0, int64_t rows, bool train, hipStream_t s);
int bn_backward(dcv_mlp* m, int l, float* dz, int64_t ld_dz, int halves, int64_t rows_half, int act, float hscale, const DropCfg& drop,
                int* blocks_out, hipStream_t s);
int bn_eval_backward(dcv_mlp* m, int l, float* dz, int64_t ld_dz, int64_t rows, int act, hipStream_t s);

// ------------------------------------------------------------------ shared by the engine's own units (mlp*.hip)
constexpr int kColsumRows = 32;    // rows per block of colsum_kernel (a block walks its rows serially: short blocks, many of them)
constexpr int kSseRows = 16;       // rows per block of ae_sse_kernel
constexpr int kStatBlockRows = 128;
constexpr int kVaeRows = 256;   // rows per block of the sampling kernels: one thread per row

struct ReduceDesc {
    const float* slab;   // [splits][count]
    const float* bpart;  // [bblocks][out]
    int64_t w_off, b_off;
    int64_t w_count;     // out*in
    int out;
    int splits, bblocks;
    int64_t w_stride, b_stride;   // floats between consecutive partials (0: dense = w_count / out).  The fused small-network
                                  // kernels pad them to multiples of 4 so that 16-byte loads work for any layer size (15-wide
                                  // layers: 810 = 54 * 15 weights per partial took the scalar walk, 15 us per reduction)
};
struct ReduceArgs {
    ReduceDesc l[2 * DCV_MAX_LAYERS];   // [0, L): the Linear layers; [L, 2 L): weight / bias of the batch normalisation behind layer l - L (empty without one)
    int L;
};
// the descriptor of Linear layer p with `splits` weight partials and `bblocks` bias partials, in its own buffers unless told otherwise
inline ReduceDesc linear_reduce_desc(const LayerPlan& p, int splits, int bblocks) {
    return ReduceDesc{p.slab, p.bpart, p.w_off, p.b_off, (int64_t)p.out * p.in, p.out, splits, bblocks, 0, 0};
}

// kind: 0 forward, 1 weight gradient, 2 input gradient (-1: any).  Every class (layer, kind) counts its own samples: the
// host may sample the kinds on different steps (dcv_mlp_profile_pause: a profiled launch costs ~7 us of command-processor
// work, so bench.py staggers them instead of stamping both layer-0 products of every step)
inline bool prof_on(const dcv_mlp* m, int layer, int kind = -1) {
    if (!(m->prof_level > 0 && !m->prof_paused && (m->prof_level > 1 || layer == 0))) return false;
    if (kind < 0) return true;
    return ((m->prof_kind_off >> kind) & 1) == 0 && m->prof_cnt[(size_t)3 * layer + kind] < m->prof_cap;
}
// which = 0: before the launch(es) of the class, 1: after.  The pair of events is offered to the block engine's launcher
// (g_launch_ev, common.h), which stamps it with the kernel's own begin / end; when the launch in between did not take it
// (the fused small-network step, a grouped launch), the events are recorded around the launch instead.
inline void prof_mark(dcv_mlp* m, int layer, int kind, int which, hipStream_t s) {
    if (!prof_on(m, layer, kind)) return;
    const size_t cls = (size_t)3 * layer + kind;
    hipEvent_t* ev = &m->prof_ev[(cls * m->prof_cap + m->prof_cnt[cls]) * 2];
    if (which == 0) {
        (void)hipEventRecord(ev[0], s);
        if (g_launch_ev.start == nullptr) g_launch_ev = LaunchEvents{ev[0], ev[1]};   // (one offer at a time: a grouped launch is bracketed by two classes)
    } else {
        m->prof_cnt[cls] += 1;
        if (g_launch_taken == ev[0]) {   // the launcher took the pair: both events carry the kernel's own times
            g_launch_taken = nullptr;
            return;
        }
        if (g_launch_ev.start == ev[0]) g_launch_ev = LaunchEvents{};
        (void)hipEventRecord(ev[1], s);
    }
}

// Deep-TICA batches.  Gathered batch (idx given): rows [0,B) are the x_t rows, rows [B,2B) the x_lag rows.
// Contiguous batch (row0 .. row0+B-1, the sequential-split / unshuffled case): x_lag of sample i IS x_t of
// sample i + lag, so the network is evaluated once on the B + lag rows row0 .. row0+B+lag-1 and both
// halves read the shared outputs -- the same numbers as two separate passes (every row goes through the
// same weights), about half the matrix work.  The gradient of a shared row is the sum of its two roles.
// (Not with dropout in a training step: the reference evaluates x_t and x_lag in two forward calls with independent masks.)
inline bool shared_rows(const dcv_mlp* m, const int64_t* idx, int batch) {
    return m->desc.model == DCV_MODEL_DEEPTICA && idx == nullptr && m->desc.lag >= 1 && m->desc.lag <= batch && !m->no_row_sharing &&
           !(m->fwd_train && (m->any_drop || m->any_bn));   // separate forward calls: independent dropout masks, separate batch statistics
}
// dropout behind Linear `layer` in the current step (off in evaluation mode)
inline DropCfg drop_cfg(const dcv_mlp* m, int layer) {
    const float p = m->desc.dropout[layer];
    if (!m->fwd_train || !(p > 0.f)) return kNoDrop;
    double t = (double)p * 4294967296.0;
    if (t > 4294967295.0) t = 4294967295.0;
    if (t < 1.0) t = 1.0;
    // rank r of a data-parallel run draws from its own stream (key word 1 offset by r * golden ratio): every rank holds
    // the same seed, and with a shared key all ranks would mask their local rows alike
    return DropCfg{(uint32_t)t, 1.f / (1.f - p), (uint32_t)(m->desc.seed & 0xFFFFFFFFull), (uint32_t)(m->desc.seed >> 32) + 0x9E3779B9u * m->drop_rank, (uint32_t)layer,
                   (uint32_t)m->cur_step};
}
inline float drop_hscale(const dcv_mlp* m, int layer) {
    const float p = m->desc.dropout[layer];
    return (m->fwd_train && p > 0.f) ? 1.f - p : 1.f;
}
inline RowMap batch_rows(const dcv_mlp* m, const int64_t* idx, int64_t row0, int batch) {
    if (m->desc.model == DCV_MODEL_DEEPTICA && !shared_rows(m, idx, batch)) return RowMap{idx, row0, batch, m->desc.lag};
    return RowMap{idx, row0, 0, 0};
}
inline int64_t rows_of(const dcv_mlp* m, const int64_t* idx, int batch) {
    if (m->desc.model != DCV_MODEL_DEEPTICA) return batch;
    return shared_rows(m, idx, batch) ? (int64_t)batch + m->desc.lag : 2 * (int64_t)batch;
}
inline int lag_offset(const dcv_mlp* m, const int64_t* idx, int batch) { return shared_rows(m, idx, batch) ? m->desc.lag : batch; }

template <class T>
int dmalloc(T** p, size_t count) {
    *p = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T));
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        return DCV_ENOMEM;
    }
    return DCV_OK;
}

// layer l + 1 can ride in the epilogue of layer l: it is narrow and layer l's output fits one column tile
inline bool head_fusion_off() {   // DCV_NO_HEAD_FUSION=1: neither the forward nor the backward fusion of a narrow layer
    static const bool off = env_is("DCV_NO_HEAD_FUSION", '1');
    return off;
}
inline bool next_layer_fusable(const dcv_mlp* m, int l) {
    if (head_fusion_off() || l + 1 >= m->L || m->any_bn) return false;
    if (m->desc.dropout[l + 1] > 0.f) return false;
    if (m->vae_d > 0 && l + 1 == m->desc.latent_layer) return false;   // the first decoder Linear reads z, sampled in between
    return m->layers[l + 1].out <= 8 && m->layers[l].out <= 128;
}

// what the layer behind Linear l hands on: the batch-normalised values when it has a normalisation, else the activations
inline float* layer_out(const dcv_mlp* m, int l) { return m->layers[l].bn ? m->layers[l].Y : m->layers[l].H; }

// What a step leaves in the engine for the calls behind it.  step_begin: the mode of its forward, and for a training forward
// the next dropout step -- ahead of the launches where they read it (forward_impl), behind a fused launch, which does not.
inline void step_begin(dcv_mlp* m, bool train) {
    m->fwd_train = train;
    if (train) m->cur_step = m->drop_step++;
}
// step_done: the path it took (dcv_mlp::last_path), its batch, and whether its loss record is written already (head_done).
// Only a fused Deep-TICA forward whose head is still to come kept its blob for the backward.
inline void step_done(dcv_mlp* m, int path, int32_t batch, bool head_done) {
    m->head_done = head_done;
    m->last_batch = batch;
    m->last_path = path;
    m->snet_fwd_valid = path == 2 && !head_done;
}

// mlp_opt.hip: the optimiser and the ordered reduction of gradient partials (slabs + bias partials -> m->grads)
void launch_fill(float* p, int64_t n, float v, int blocks, int threads, hipStream_t s);   // p[0, n) = v
int reset_opt_state(dcv_mlp* m, hipStream_t s);
ReduceArgs reduce_args_of(const dcv_mlp* m, const ReduceArgsView& v);
int launch_reduce(dcv_mlp* m, const ReduceArgs& ra, int l0, int l1, hipStream_t s);   // layers [l0, l1), no update
int reduce_upper(dcv_mlp* m, const ReduceArgs& ra, bool fuse_opt, bool* done, hipStream_t s);
struct OptArgs;   // reduce_quad.h
int ride_upper(dcv_mlp* m, const ReduceArgs& ra, const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t k_chunk,
               const EpiSlab& epi, OptArgs* oa, hipStream_t s);   // 1 = not applicable
int finish_grads(dcv_mlp* m, const ReduceArgs& ra, bool fuse_opt, bool upper_done, hipStream_t s, const OptArgs* ridden = nullptr);
int apply_impl(dcv_mlp* m, void* stream);
// mlp_heads.hip: launchers of the loss-head kernels
int launch_sum_partials(const double* part, int nblocks, int width, double* out, hipStream_t s);
int launch_log_advance(int* log_count, int n, hipStream_t s);   // the log counter + n behind a batched launch (loss_head.h: log_member)
int stats_rows_per_block(int64_t batch);
int tica_stats(dcv_mlp* m, const float* F, int64_t ldf, int batch, int lag_off, int fuse_head, bool* head_ran, hipStream_t s);
bool tica_stats_groupable(int d);
int tica_stats_group(dcv_mlp* m, const float* F, int64_t ldf, int64_t f_stride, int batch, int lag_off, int blocks, int members, double* part,
                     unsigned* tickets, hipStream_t s);
int loss_record(dcv_mlp* m, int64_t global_batch, bool train, bool head_in_bwd, hipStream_t s);
bool head_fusable(const dcv_mlp* m);
int head_backward(dcv_mlp* m, int64_t R, int batch, int lag_off, float* dZ, int* blocks, hipStream_t s);
int ae_sse(dcv_mlp* m, const float* Y, int64_t ldy, const float* Xn, int64_t ldx, const RowMap& rm, int64_t R, int batch, bool fuse_head, hipStream_t s);
int loss_gradient(dcv_mlp* m, const float* Y, int64_t ldy, const float* Xn, int64_t ldx, const RowMap& rm, int64_t R, int batch, int lag_off,
                  int64_t global_batch, int act, float* dZ, const DropCfg& drop, float hscale, hipStream_t s);
// mlp.hip: the steps the passes of mlp_passes.hip are built on
int run_forward(dcv_mlp* m, const float* Xn, int64_t ld, const RowMap& rows_map, int64_t rows, int n_run, hipStream_t s, bool for_backward = false);
bool peek_noise(dcv_mlp* m, int64_t rows);
int forward_impl(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t train, void* stream,
                 int fuse_head = 0);
int backward_impl(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int64_t global_batch, int32_t train,
                  void* stream, bool fuse_opt = false);
}  // namespace dcv

// MLP engine, the passes built on its steps: several training steps per call, the validation pass (fused small-network
// launches, the block engine's grouped pass), the data-parallel step, inference and the input-sensitivity pass.
#include "mlp_state.h"
#include <utility>

using namespace dcv;

// batch j of a pass: the samples [j * batch, (j + 1) * batch) of the index list, or of the row range when there is none
struct BatchSlice { const int64_t* idx; int64_t row0; };
static BatchSlice batch_slice(const int64_t* idx_d, int64_t row0, int64_t j, int32_t batch) {
    return BatchSlice{idx_d ? idx_d + j * batch : nullptr, idx_d ? row0 : row0 + j * batch};
}

// nsteps consecutive training steps in one call: step j takes samples [j * batch, (j + 1) * batch) of the index list / the row
// range, exactly as nsteps calls of dcv_mlp_train_step would (same launches, same records).  What it removes is the caller's
// per-step cost: a small-network step is ~30 - 40 us of device time and a Python caller spends 10 - 30 us per call on some
// hosts (bench.py c2: 46 us per step from Python against 39 us of launches) -- the epoch loop of a fit belongs on this side
// of the boundary.
extern "C" int dcv_mlp_train_steps(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t nsteps,
                                   void* stream) {
    DCV_REQUIRE(m && Xn_d, "dcv_mlp_train_steps: null argument");
    DCV_REQUIRE(nsteps >= 0 && batch >= 1, "dcv_mlp_train_steps: nsteps=%d batch=%d", nsteps, batch);
    for (int32_t j = 0; j < nsteps; ++j) {
        const BatchSlice b = batch_slice(idx_d, row0, j, batch);
        const int rc = dcv_mlp_train_step(m, Xn_d, ld, b.idx, b.row0, batch, stream);
        if (rc) return rc;
    }
    return DCV_OK;
}

// ---- grouped validation pass of the block engine
// DCV_EVAL_GROUP (read once per process): 0 = dcv_mlp_eval_steps steps batch by batch on the block engine, as it did before
// the grouped pass existed; N >= 2 = at most N members per launch; unset = kEvalBatchesPerLaunch
static int eval_group_limit() {
    static const int lim = [] {
        const char* e = getenv("DCV_EVAL_GROUP");
        if (!e || !e[0]) return kEvalBatchesPerLaunch;
        const int v = atoi(e);
        return v <= 1 ? 0 : (v < kEvalBatchesPerLaunch ? v : kEvalBatchesPerLaunch);
    }();
    return lim;
}
// The workspace for `members` batches of R rows (`batch` pairs) each: per layer [members][R][ldh] outputs, then per member a
// tail workspace of the engine's size (TailWs) and the statistics partials, then the tickets (8 tail tickets per member,
// one statistics ticket per member).  Every region starts on a 256-byte boundary.
struct EvalGroupLayout {
    size_t act[DCV_MAX_LAYERS], tail, spart, tickets, ticket_bytes, bytes;
    size_t stat_tickets;   // index of the first statistics ticket
    int stat_blocks;
};
static EvalGroupLayout eval_group_layout(const dcv_mlp* m, int members, int64_t R, int batch) {
    EvalGroupLayout lo{};
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off += align_up(n, 256); return at; };
    for (int l = 0; l < m->L; ++l) lo.act[l] = take((size_t)members * R * m->layers[l].ldh * sizeof(float));
    lo.tail = take(m->tail.ws ? (size_t)members * m->tail.cap * sizeof(float) : 0);
    lo.stat_blocks = (int)cdiv(batch, stats_rows_per_block(batch));
    lo.spart = take((size_t)members * lo.stat_blocks * m->stats_len * sizeof(double));
    lo.stat_tickets = (size_t)members * 8;
    lo.ticket_bytes = (lo.stat_tickets + members) * sizeof(unsigned);
    lo.tickets = take(lo.ticket_bytes);
    lo.bytes = off;
    return lo;
}
// Up to `want` consecutive evaluation batches (batch j = the pairs [j * batch, (j + 1) * batch) behind idx_d / row0) as ONE
// launch per layer and one statistics launch: the batches of a validation pass do not depend on each other (the weights
// stand still), and one batch of a few thousand rows cannot fill the chip with large tiles -- a group can.  Every member is
// computed exactly as dcv_mlp_eval_step computes it (gemm_kernels.h: launch_gemm_group; tica_stats_rows_group_kernel), into
// its own segment of a workspace: the engine's activation buffers, sign masks and gradients are not touched.
// Returns the members launched (>= 2), 0 when the group form does not apply (the caller steps), < 0 on error.
static int eval_group(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int want, hipStream_t s) {
    if (m->desc.model != DCV_MODEL_DEEPTICA || !tica_stats_groupable(m->d_out) || m->any_drop || m->any_bn || m->eval_ws.failed) return 0;
    if (!(m->snet_dt_tried && m->snet_dt == nullptr)) return 0;   // a single step might take the fused small-network kernels
    for (int l = 0; l < m->L; ++l)   // a fused narrow layer of 5 - 8 outputs has no grouped instantiation
        if (l + 1 < m->L && next_layer_fusable(m, l)) {
            if (m->layers[l + 1].out > 4) return 0;
            ++l;
        }
    int members = want < eval_group_limit() ? want : eval_group_limit();
    const bool was_train = m->fwd_train;
    m->fwd_train = false;   // (rows_of / batch_rows ask)
    const int64_t R = rows_of(m, idx_d, batch);
    const RowMap rm = batch_rows(m, idx_d, row0, batch);
    const int lag_off = lag_offset(m, idx_d, batch);
    m->fwd_train = was_train;
    const size_t per_member = eval_group_layout(m, 2, R, batch).bytes - eval_group_layout(m, 1, R, batch).bytes;
    if ((size_t)members * per_member > kEvalGroupBudgetBytes) members = (int)(kEvalGroupBudgetBytes / per_member);
    if (members < 2) return 0;
    // The first grouped pass of an engine allocates here (a fit: inside its first validation pass, once: a hipMalloc of up to
    // kEvalGroupBudgetBytes, about a millisecond); later passes of the same shape find the workspace as it is.  Only a pass
    // with more members or longer batches than any before frees it (hipFree waits for the device) and allocates again.
    EvalGroupWs& ws = m->eval_ws;
    const bool same = ws.base != nullptr && ws.members >= members && ws.rows == R && ws.batch == batch;   // (a smaller group uses the first segments)
    const EvalGroupLayout lo = eval_group_layout(m, same ? ws.members : members, R, batch);
    if (!same) {
        if (ws.bytes < lo.bytes) {
            if (ws.base) (void)hipFree(ws.base);
            ws = EvalGroupWs{};
            void* p = nullptr;
            if (hipMalloc(&p, lo.bytes) != hipSuccess) {
                (void)hipGetLastError();
                ws.failed = true;   // not an error: the pass steps batch by batch
                return 0;
            }
            ws.base = static_cast<char*>(p);
            ws.bytes = lo.bytes;
        }
        // the tickets of this layout (zero between launches from here on: every last arriver resets its own)
        DCV_CHECK_HIP(hipMemsetAsync(ws.base + lo.tickets, 0, lo.ticket_bytes, s));
        ws.members = members;
        ws.rows = R;
        ws.batch = batch;
    }
    auto act_of = [&](int l) { return reinterpret_cast<float*>(ws.base + lo.act[l]); };
    unsigned* tickets = reinterpret_cast<unsigned*>(ws.base + lo.tickets);
    TailWs tw{};
    if (m->tail.ws) tw = TailWs{reinterpret_cast<float*>(ws.base + lo.tail), tickets, m->tail.cap, m->tail.max_tiles_n};
    g_launch_ev = LaunchEvents{};
    for (int l = 0; l < m->L; ++l) {
        const LayerPlan& p = m->layers[l];
        GroupShift g;
        g.out_rows = R;
        g.tail_floats = m->tail.cap;
        g.tail_tickets = 8;
        Operand A;
        if (l == 0) {
            A = make_operand(Xn_d, ld, p.in, rm);
            g.a_rows = batch;
        } else {
            A = make_operand(act_of(l - 1), m->layers[l - 1].ldh, p.in);
            g.a_floats = R * m->layers[l - 1].ldh;
        }
        Operand B = make_operand(m->params + p.w_off, p.in, p.in);
        float* H = act_of(l);
        int rc;
        if (l + 1 < m->L && next_layer_fusable(m, l)) {   // as run_forward: the narrow Linear behind this layer rides in its epilogue
            const LayerPlan& nx = m->layers[l + 1];
            const bool vec = quad_ok(H, p.ldh) && quad_ok(m->params + p.b_off, 4) && quad_ok(m->params + nx.w_off, nx.in);
            EpiBiasActHead<4> epi{H, p.ldh, m->params + p.b_off, p.act, vec, m->params + nx.w_off, nx.in, m->params + nx.b_off, nx.out, nx.act, act_of(l + 1), nx.ldh};
            rc = gemm_nt_head4_group(A, B, R, p.out, p.in, epi, g, members, &tw, s);
            ++l;
        } else {
            EpiBiasAct epi{H, p.ldh, m->params + p.b_off, p.act, quad_ok(H, p.ldh) && quad_ok(m->params + p.b_off, 4)};
            rc = gemm_nt_bias_act_group(A, B, R, p.out, p.in, epi, g, members, &tw, s);
        }
        if (rc < 0) return rc;
        if (rc != DCV_OK) return 0;   // (scalar-load operands: nothing of the group reached the log)
    }
    const LayerPlan& last = m->layers[m->L - 1];
    const int rcs = tica_stats_group(m, act_of(m->L - 1), last.ldh, R * last.ldh, batch, lag_off, lo.stat_blocks, members,
                                     reinterpret_cast<double*>(ws.base + lo.spart), tickets + lo.stat_tickets, s);
    if (rcs) return rcs;
    // the engine as the last single evaluation step would leave it
    for (int l = 0; l < m->L; ++l) m->layers[l].mask_rows = -1;
    step_begin(m, false);
    step_done(m, 0, batch, false);
    return members;
}

// nbatches consecutive evaluation steps -- batch j = samples [j * batch, (j + 1) * batch) of the index list (idx_d + j * batch)
// or of the row range (row0 + j * batch) -- with one loss record each, in batch order: the records dcv_mlp_eval_step would
// append one call at a time.  A small network (snet.hip / snet_dt.hip) evaluates up to kEvalBatchesPerLaunch batches per
// launch -- a validation pass is then one launch instead of one (autoencoder) or one (Deep-TICA) per batch, each of which is
// mostly launch latency and weight staging.  The block engine evaluates a Deep-TICA network (no dropout, no batch
// normalisation, at most 4 outputs) in groups of up to kEvalBatchesPerLaunch batches, as many as kEvalGroupBudgetBytes of
// workspace hold: one launch per layer with a member per batch (eval_group), full groups first, then the rest (a single
// batch left over takes dcv_mlp_eval_step); DCV_EVAL_GROUP=0 turns that off.  Every other engine runs the steps one after
// the other.  The records are bit for bit those of the single steps on every path.
extern "C" int dcv_mlp_eval_steps(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int32_t nbatches,
                                  void* stream) {
    DCV_REQUIRE(m && Xn_d, "dcv_mlp_eval_steps: null argument");
    DCV_REQUIRE(nbatches >= 0, "dcv_mlp_eval_steps: nbatches=%d", nbatches);
    DCV_REQUIRE(batch >= 1 && batch <= m->desc.max_batch, "dcv_mlp_eval_steps: batch=%d exceeds max_batch=%d", batch, m->desc.max_batch);
    DCV_REQUIRE(ld >= m->desc.dims[0], "dcv_mlp_eval_steps: ld=%lld < F=%d", (long long)ld, m->desc.dims[0]);
    DCV_REQUIRE(m->log && m->log_cap > 0, "dcv_mlp_eval_steps: call dcv_mlp_reset_log first");
    hipStream_t s = as_stream(stream);
    int32_t j = 0;
    m->last_eval_group = 0;
    bool grouped = false;
    while (j < nbatches) {
        const BatchSlice b = batch_slice(idx_d, row0, j, batch);
        int nb = nbatches - j < kEvalBatchesPerLaunch ? nbatches - j : kEvalBatchesPerLaunch;
        const int left = nbatches - j;
        int rc = 1;
        if (nb > 1 && !m->any_drop && !m->any_bn && !prof_on(m, 0)) {   // (a profiled run samples single steps)
            g_launch_ev = LaunchEvents{};
            int path = 0;
            if ((m->desc.model == DCV_MODEL_AE || m->desc.model == DCV_MODEL_VAE) && !(m->snet_tried && m->snet == nullptr)) {
                const int tr = snet_ae_tile_rows(m, batch);
                const int64_t per = cdiv((int64_t)batch, tr > 0 ? tr : 16);   // workgroups per batch
                while (nb > 1 && per * nb > kEvalWorkgroupsPerLaunch) --nb;
                if (m->vae_d > 0)   // VAE: as many batches as the noise buffer still covers (batch j takes eps rows [j * batch, (j + 1) * batch))
                    while (nb > 1 && !peek_noise(m, (int64_t)nb * batch)) --nb;
                if (nb > 1) rc = snet_ae_step(m, Xn_d, ld, RowMap{b.idx, b.row0, 0, 0}, batch, batch, 0, nullptr, s, true, nb);
                if (rc == DCV_OK && m->vae_d > 0) m->noise_pos += (int64_t)nb * batch;
                path = 1;
            } else if (m->desc.model == DCV_MODEL_DEEPTICA && !(m->snet_dt_tried && m->snet_dt == nullptr)) {
                const int64_t per = cdiv((int64_t)batch, 8);   // (an upper bound of the workgroups per batch: tiles of >= 8 pairs)
                while (nb > 1 && per * nb > kEvalWorkgroupsPerLaunch) --nb;
                if (nb > 1) rc = snet_dt_forward(m, Xn_d, ld, b.idx, b.row0, batch, 2, false, s, nb);
                path = 2;
            }
            if (rc < 0) return rc;
            if (rc == DCV_OK) {   // the launch wrote the nb records (Deep-TICA: through the loss head in its last blocks)
                step_begin(m, false);
                step_done(m, path, batch, m->desc.model == DCV_MODEL_DEEPTICA);
                j += nb;
                continue;
            }
            if (left > 1 && eval_group_limit() > 0) {   // the block engine: groups of batches, one launch per layer
                const int done = eval_group(m, Xn_d, ld, b.idx, b.row0, batch, left, s);
                if (done < 0) return done;
                if (done > 0) {
                    if (!grouped) m->last_eval_group = done;
                    grouped = true;
                    j += done;
                    continue;
                }
            }
        }
        rc = dcv_mlp_eval_step(m, Xn_d, ld, b.idx, b.row0, batch, stream);
        if (rc) return rc;
        j += 1;
    }
    return DCV_OK;
}

// ---- data-parallel step: the whole sequence behind one entry point, the collectives through a host callback
namespace {
struct DpTrampoline {
    dcv_mlp* m;
    dcv_allreduce_fn fn;
    void* user;
    int rc;
};
void dp_upper_cb(void* p) {
    DpTrampoline* t = static_cast<DpTrampoline*>(p);
    const int64_t off = t->m->layers[1].w_off;
    t->rc = t->fn(t->user, t->m->grads + off, t->m->n_params - off, DCV_DTYPE_F32, DCV_DP_UPPER_START);
}
}  // namespace

// Data-parallel autoencoder step through the fused small-network launch (snet.hip): the loss gradient of a row needs nothing
// from the other ranks (the scale 2 / (global batch * F) is known up front), so the whole local forward + backward is the
// one launch of the single-GPU step; then the squared-error sum is all-reduced and logged, the gradient partials are
// reduced, the gradient buffer all-reduced, the update applied.  1 = not applicable.
static int dp_ae_fused(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch, int64_t global_batch,
                       int32_t train, dcv_allreduce_fn fn, void* user, void* stream) {
    if (m->desc.model != DCV_MODEL_AE || m->any_drop || m->any_bn || (m->snet_tried && m->snet == nullptr)) return 1;
    if (!(Xn_d && batch >= 1 && batch <= m->desc.max_batch && ld >= m->desc.dims[0] && m->log && m->log_cap > 0 && global_batch >= batch)) return 1;
    hipStream_t s = as_stream(stream);
    g_launch_ev = LaunchEvents{};
    ReduceArgsView v;
    prof_mark(m, 0, 0, 0, s);
    prof_mark(m, 0, 1, 0, s);
    int rc = snet_ae_step(m, Xn_d, ld, RowMap{idx_d, row0, 0, 0}, batch, global_batch, train, &v, s, false);
    if (rc) return rc;
    prof_mark(m, 0, 0, 1, s);
    prof_mark(m, 0, 1, 1, s);
    step_begin(m, train != 0);
    step_done(m, 1, batch, false);
    if (fn(user, m->stats, m->stats_len, DCV_DTYPE_F64, DCV_DP_STATS) != 0) {
        set_error("dcv_mlp_dp_step: the all-reduce callback failed (statistics)");
        return DCV_ECALLBACK;
    }
    rc = loss_record(m, global_batch, train != 0, false, s);
    if (rc || !train) return rc;
    rc = launch_reduce(m, reduce_args_of(m, v), 0, m->L, s);
    if (rc) return rc;
    if (fn(user, m->grads, m->n_params, DCV_DTYPE_F32, DCV_DP_GRADS) != 0) {
        set_error("dcv_mlp_dp_step: the all-reduce callback failed (gradients)");
        return DCV_ECALLBACK;
    }
    return apply_impl(m, stream);
}

extern "C" int dcv_mlp_dp_step(dcv_mlp* m, const float* Xn_d, int64_t ld, const int64_t* idx_d, int64_t row0, int32_t batch,
                               int64_t global_batch, int32_t train, int32_t overlap, dcv_allreduce_fn fn, void* user, void* stream) {
    DCV_REQUIRE(m && fn, "dcv_mlp_dp_step: null argument");
    if (m->vae_d > 0 && global_batch != batch) {
        set_error("dcv_mlp_dp_step: the variational autoencoder is not implemented for data-parallel fits (global batch %lld != local batch %d); "
                  "fit it on one GPU", (long long)global_batch, batch);
        return DCV_EINVAL;
    }
    const int rcf = dp_ae_fused(m, Xn_d, ld, idx_d, row0, batch, global_batch, train, fn, user, stream);
    if (rcf != 1) return rcf;
    // Batch normalisation normalises with the rows of ONE forward call: in a frame-sharded step that would be each rank's
    // local rows, the running statistics would drift apart between the ranks, and N ranks would no longer equal one process
    // on the union batch (which every other part of this step guarantees).  Refused rather than silently different.
    if (m->any_bn && global_batch != batch) {
        set_error("dcv_mlp_dp_step: batch normalisation is not implemented for data-parallel fits (global batch %lld != local batch %d: "
                  "the normalisation would use each rank's local rows only); fit on one GPU or drop `batchnorm`", (long long)global_batch, batch);
        return DCV_EINVAL;
    }
    // whatever fails from here on, a reduction started with DCV_DP_UPPER_START must be joined before the caller gets the
    // gradient buffer back: every exit below goes through fail()
    bool started = false;
    auto fail = [&](int rc) {
        if (started) (void)fn(user, nullptr, 0, DCV_DTYPE_F32, DCV_DP_WAIT);
        return rc;
    };
    int rc = forward_impl(m, Xn_d, ld, idx_d, row0, batch, train, stream, 0);
    if (rc) return rc;
    if (fn(user, m->stats, m->stats_len, DCV_DTYPE_F64, DCV_DP_STATS) != 0) {
        set_error("dcv_mlp_dp_step: the all-reduce callback failed (statistics)");
        return DCV_ECALLBACK;
    }
    if (!train) return backward_impl(m, Xn_d, ld, idx_d, row0, batch, global_batch, 0, stream);
    if (overlap && m->L > 1) {
        // the gradients of layers 1.. are reduced and handed to the callback before the layer-0 weight gradient is
        // enqueued (dcv_mlp_set_upper_grads_callback): their exchange runs under the largest product of the step
        DpTrampoline t{m, fn, user, 0};
        void (*keep_cb)(void*) = m->upper_cb;
        void* keep_user = m->upper_cb_user;
        m->upper_cb = dp_upper_cb;
        m->upper_cb_user = &t;
        started = true;   // (the trampoline may have started the exchange even when the backward fails behind it)
        rc = backward_impl(m, Xn_d, ld, idx_d, row0, batch, global_batch, 1, stream);
        m->upper_cb = keep_cb;
        m->upper_cb_user = keep_user;
        if (rc) return fail(rc);
        if (t.rc != 0 || fn(user, m->grads, m->layers[1].w_off, DCV_DTYPE_F32, DCV_DP_GRADS) != 0) {
            set_error("dcv_mlp_dp_step: the all-reduce callback failed (gradients)");
            return fail(DCV_ECALLBACK);
        }
        started = false;
        if (fn(user, nullptr, 0, DCV_DTYPE_F32, DCV_DP_WAIT) != 0) {
            set_error("dcv_mlp_dp_step: the all-reduce callback failed (join)");
            return DCV_ECALLBACK;
        }
    } else {
        void (*keep_cb)(void*) = m->upper_cb;
        m->upper_cb = nullptr;
        rc = backward_impl(m, Xn_d, ld, idx_d, row0, batch, global_batch, 1, stream);
        m->upper_cb = keep_cb;
        if (rc) return rc;
        if (fn(user, m->grads, m->n_params, DCV_DTYPE_F32, DCV_DP_GRADS) != 0) {
            set_error("dcv_mlp_dp_step: the all-reduce callback failed (gradients)");
            return DCV_ECALLBACK;
        }
    }
    return apply_impl(m, stream);
}

extern "C" int dcv_mlp_infer(dcv_mlp* m, const float* Xn_d, int64_t n, int64_t ld, const float* tmean_d, const float* tevecs_d,
                             const float* pmean_d, const float* prange_d, float* out_d, float* minmax_d, void* stream) {
    DCV_REQUIRE(m && Xn_d && n >= 1, "dcv_mlp_infer: bad arguments");
    DCV_REQUIRE(n <= m->rows_cap, "dcv_mlp_infer: n=%lld exceeds the row capacity %lld (chunk the call)", (long long)n, (long long)m->rows_cap);
    DCV_REQUIRE((tmean_d == nullptr) == (tevecs_d == nullptr), "dcv_mlp_infer: tmean/tevecs must come together");
    hipStream_t s = as_stream(stream);
    const int n_run = m->desc.model == DCV_MODEL_DEEPTICA ? m->L : m->desc.latent_layer;
    const RowMap rm = identity_rows();
    m->fwd_train = false;
    int rc = run_forward(m, Xn_d, ld, rm, n, n_run, s);
    if (rc) return rc;
    const LayerPlan& last = m->layers[n_run - 1];
    const int d = m->vae_d > 0 ? m->vae_d : last.out;   // VAE: the CV is the mean head, the first d of the 2d head columns
    // y = (h - tmean) @ tevecs ; out = (y - pmean) / prange   -- the linear projection kernel
    return dcv_project_linear(layer_out(m, n_run - 1), n, d, last.ldh, tmean_d ? tmean_d : m->zeros_d, m->ones_d, tevecs_d ? tevecs_d : m->ident, d,
                              nullptr, pmean_d, prange_d, out_d, minmax_d, m->proj_ws, m->proj_ws_bytes, stream);
}

namespace dcv {
// dZ_last[r][c] = g[c] * act'(H_last[r][c]): the gradient of s = sum_j cv_j w.r.t. the network output is the
// same vector for every frame (the layers after the network are affine)
__global__ __launch_bounds__(256) void seed_grad_kernel(const float* __restrict__ H, int64_t ldh, int64_t rows, int d, int act,
                                                        const float* __restrict__ g, float* __restrict__ dZ, int64_t ld_dz) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * d) return;
    const int64_t r = i / d;
    const int c = (int)(i - r * d);
    dZ[r * ld_dz + c] = g[c] * act_grad_from_out(act, H[r * ldh + c]);
}

// part[block][c] = sum over the block's rows of |G[r][c]| * scale[c] (float64, rows in index order)
constexpr int kAbsRows = 256;
__global__ __launch_bounds__(256) void abs_colsum_kernel(const float* __restrict__ G, int64_t ldg, int64_t rows, int F,
                                                         const float* __restrict__ scale, double* __restrict__ part) {
    const int64_t r0 = (int64_t)blockIdx.x * kAbsRows;
    const int64_t r1 = r0 + kAbsRows < rows ? r0 + kAbsRows : rows;
    for (int c = threadIdx.x; c < F; c += 256) {
        double acc = 0.0;
        const double sc = (double)scale[c];
        for (int64_t r = r0; r < r1; ++r) acc += fabs((double)G[r * ldg + c]) * sc;
        part[(int64_t)blockIdx.x * F + c] = acc;
    }
}
}  // namespace dcv

// Input-gradient pass of the sensitivity analysis (reference cv_calculator.py:1893-1921 ->
// mlcolvar.explain.sensitivity_analysis, metric "mean_abs_val"): for the rows given,
// sens[i] = sum_r | d(sum_j cv_j)/d xn[r][i] | * scale[i], where the layers behind the network (TICA,
// post-normalisation) enter through the constant vector g = d(sum_j cv_j)/d(network output).
extern "C" size_t dcv_mlp_input_sensitivity_workspace(const dcv_mlp* m, int64_t n) {
    if (!m || n < 1) return 0;
    const size_t F = (size_t)m->desc.dims[0];
    return align_up((size_t)n * F * sizeof(float), 256) + (size_t)cdiv(n, kAbsRows) * F * sizeof(double);
}

extern "C" int dcv_mlp_input_sensitivity(dcv_mlp* m, const float* Xn_d, int64_t n, int64_t ld, const float* gout_d,
                                         const float* scale_d, double* sens_d, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    DCV_REQUIRE(m && Xn_d && gout_d && scale_d && sens_d && workspace, "dcv_mlp_input_sensitivity: null argument");
    DCV_REQUIRE(n >= 1 && n <= m->rows_cap, "dcv_mlp_input_sensitivity: n=%lld outside [1, %lld] (chunk the call)", (long long)n,
                (long long)m->rows_cap);
    DCV_REQUIRE(workspace_bytes >= dcv_mlp_input_sensitivity_workspace(m, n), "dcv_mlp_input_sensitivity: workspace too small");
    hipStream_t s = as_stream(stream);
    const int F = m->desc.dims[0];
    DCV_REQUIRE(ld >= F, "dcv_mlp_input_sensitivity: ld=%lld < F=%d", (long long)ld, F);
    const int n_run = m->desc.model == DCV_MODEL_DEEPTICA ? m->L : m->desc.latent_layer;
    m->fwd_train = false;
    int rc = run_forward(m, Xn_d, ld, identity_rows(), n, n_run, s);
    if (rc) return rc;
    const LayerPlan& last = m->layers[n_run - 1];
    float* dz_cur = m->dZ[0];
    float* dz_nxt = m->dZ[1];
    hipLaunchKernelGGL(seed_grad_kernel, dim3((unsigned)cdiv(n * last.out, 256)), dim3(256), 0, s, (const float*)layer_out(m, n_run - 1), last.ldh, n,
                       last.out, last.bn ? DCV_ACT_NONE : last.act, gout_d, dz_cur, m->ld_dz);
    DCV_CHECK_LAUNCH();
    if (last.bn) {   // evaluation-mode normalisation: a per-column scale, then the activation derivative of the Linear underneath
        rc = bn_eval_backward(m, n_run - 1, dz_cur, m->ld_dz, n, last.act, s);
        if (rc) return rc;
    }
    for (int l = n_run - 1; l >= 1; --l) {   // dZ_{l-1} = (dZ_l W_l) * act'(H_{l-1})
        LayerPlan& p = m->layers[l];
        LayerPlan& q = m->layers[l - 1];
        Operand Ad = make_operand(dz_cur, m->ld_dz, p.out);
        Operand Bd = make_operand(m->params + p.w_off, p.in, p.in);
        EpiActGrad eg{dz_nxt, m->ld_dz, q.H, q.ldh, q.bn ? DCV_ACT_NONE : q.act, q.bpart, q.out, quad_ok(dz_nxt, m->ld_dz) && quad_ok(q.H, q.ldh)};
        int bblocks = 0;
        rc = gemm_nn_act_grad(Ad, Bd, n, p.in, p.out, eg, s, &bblocks, nullptr);
        if (rc) return rc;
        if (q.bn) {
            rc = bn_eval_backward(m, l - 1, dz_nxt, m->ld_dz, n, q.act, s);
            if (rc) return rc;
        }
        std::swap(dz_cur, dz_nxt);
    }
    float* G = static_cast<float*>(workspace);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + align_up((size_t)n * F * sizeof(float), 256));
    {   // dXn = dZ_0 W_0
        const LayerPlan& p = m->layers[0];
        Operand Ad = make_operand(dz_cur, m->ld_dz, p.out);
        Operand Bd = make_operand(m->params + p.w_off, p.in, p.in);
        EpiStore es{G, F, quad_ok(G, F)};
        rc = gemm_nn_store(Ad, Bd, n, p.in, p.out, es, s);
        if (rc) return rc;
    }
    const int nb = (int)cdiv(n, kAbsRows);
    hipLaunchKernelGGL(abs_colsum_kernel, dim3(nb), dim3(256), 0, s, G, (int64_t)F, n, F, scale_d, part);
    DCV_CHECK_LAUNCH();
    return launch_sum_partials(part, nb, F, sens_d, s);
}

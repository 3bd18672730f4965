// MLP engine, optimiser unit: the torch.optim single-tensor updates and the ordered reduction of the gradient partials
// (split-K weight slabs, bias column sums) that ends every backward pass -- on one GPU with the update fused in.
#include "mlp_state.h"
#include "reduce_quad.h"
#include <math.h>

namespace dcv {

static inline int64_t rd_wstride(const ReduceDesc& d) { return d.w_stride > 0 ? d.w_stride : d.w_count; }
static inline int64_t rd_bstride(const ReduceDesc& d) { return d.b_stride > 0 ? d.b_stride : (int64_t)d.out; }

__global__ __launch_bounds__(256) void optimizer_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                        float* __restrict__ s2, float* __restrict__ s3, int64_t n, OptArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) opt_update(i, g[i], p, s1, s2, s3, a);
}

// grads[w] = sum_s slab[s][w] ; grads[b] = sum_blk bpart[blk][b].  A block covers 64 consecutive
// elements; its 16 waves take the partials q = wave, wave + 16, ... (coalesced 256-byte reads)
// and are combined in wave order: float64 accumulation, fixed order, deterministic.
constexpr int kRedWaves = 16;
// fuse != 0 (one-GPU training step, nothing to all-reduce in between): the thread that finishes a gradient element
// applies the optimiser update to its parameter at once -- one launch less per step.
__global__ __launch_bounds__(64 * kRedWaves) void reduce_grads_kernel(ReduceArgs a, float* __restrict__ grads, float scale, int fuse,
                                                                      float* __restrict__ params, float* __restrict__ s1,
                                                                      float* __restrict__ s2, float* __restrict__ s3, OptArgs oa) {
    __shared__ double s_red[kRedWaves][64];
    const int l = blockIdx.y;
    const ReduceDesc& d = a.l[l];
    const int64_t total = d.w_count + d.out;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < total; base += (int64_t)gridDim.x * 64) {
        const int64_t i = base + lane;
        double s = 0.0;
        if (i < d.w_count) {
            const float* p = d.slab + i;
#pragma unroll 8
            for (int q = wave; q < d.splits; q += kRedWaves) s += (double)p[(int64_t)q * (d.w_stride > 0 ? d.w_stride : d.w_count)];
        } else if (i < total) {
            const float* p = d.bpart + (i - d.w_count);
#pragma unroll 8
            for (int q = wave; q < d.bblocks; q += kRedWaves) s += (double)p[(int64_t)q * (d.b_stride > 0 ? d.b_stride : (int64_t)d.out)];
        }
        s_red[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && i < total) {
            double tot = 0.0;
#pragma unroll
            for (int w = 0; w < kRedWaves; ++w) tot += s_red[w][lane];
            const float g = (float)(tot * (double)scale);
            const int64_t pidx = i < d.w_count ? d.w_off + i : d.b_off + (i - d.w_count);
            grads[pidx] = g;
            if (fuse) opt_update(pidx, g, params, s1, s2, s3, oa);
        }
        __syncthreads();
    }
}

// The same reduction for small split counts (small batches: the 16-wave form above spends a 1024-thread block on 64
// outputs and a handful of partials): a block covers 64 consecutive elements, its four waves take the partials
// q = wave, wave + 4, ... (independent loads, eight in flight per thread: a serial walk over the 257 partials of the
// fused last-layer pass cost 64 us of load latency) and are combined in wave order; float64, fixed order, optional
// fused optimiser update.
__global__ __launch_bounds__(256) void reduce_grads_small_kernel(ReduceArgs a, float* __restrict__ grads, float scale, int fuse,
                                                                 float* __restrict__ params, float* __restrict__ s1,
                                                                 float* __restrict__ s2, float* __restrict__ s3, OptArgs oa) {
    __shared__ double s_red[4][64];
    const ReduceDesc& d = a.l[blockIdx.y];
    const int64_t total = d.w_count + d.out;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t base = (int64_t)blockIdx.x * 64; base < total; base += (int64_t)gridDim.x * 64) {
        const int64_t i = base + lane;
        double s = 0.0;
        if (i < d.w_count) {
            const float* p = d.slab + i;
#pragma unroll 8
            for (int q = wave; q < d.splits; q += 4) s += (double)p[(int64_t)q * (d.w_stride > 0 ? d.w_stride : d.w_count)];
        } else if (i < total) {
            const float* p = d.bpart + (i - d.w_count);
#pragma unroll 8
            for (int q = wave; q < d.bblocks; q += 4) s += (double)p[(int64_t)q * (d.b_stride > 0 ? d.b_stride : (int64_t)d.out)];
        }
        s_red[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && i < total) {
            const double tot = ((s_red[0][lane] + s_red[1][lane]) + s_red[2][lane]) + s_red[3][lane];
            const float g = (float)(tot * (double)scale);
            const int64_t pidx = i < d.w_count ? d.w_off + i : d.b_off + (i - d.w_count);
            grads[pidx] = g;
            if (fuse) opt_update(pidx, g, params, s1, s2, s3, oa);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void reduce_grads_quad_kernel(QuadArgs a, float* __restrict__ grads, float scale, int fuse,
                                                                float* __restrict__ params, float* __restrict__ s1,
                                                                float* __restrict__ s2, float* __restrict__ s3, OptArgs oa) {
    __shared__ double s_red[1024];
    int l = 0;
    while (l + 1 < a.n && (int)blockIdx.x >= a.it[l + 1].blk0) ++l;   // uniform
    const QuadItem& d = a.it[l];
    const int blk = (int)blockIdx.x - d.blk0;
    if (d.groups == 16) reduce_quad_block<16>(d, blk, grads, scale, fuse, params, s1, s2, s3, oa, s_red);
    else reduce_quad_block<4>(d, blk, grads, scale, fuse, params, s1, s2, s3, oa, s_red);
}

__global__ void fill_kernel(float* p, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

void launch_fill(float* p, int64_t n, float v, int blocks, int threads, hipStream_t s) {
    hipLaunchKernelGGL(fill_kernel, dim3(blocks), dim3(threads), 0, s, p, n, v);
}

// optimiser state as a freshly constructed torch optimiser holds it
int reset_opt_state(dcv_mlp* m, hipStream_t s) {
    const size_t bytes = m->n_params * sizeof(float);
    DCV_CHECK_HIP(hipMemsetAsync(m->adam_m, 0, bytes, s));
    DCV_CHECK_HIP(hipMemsetAsync(m->adam_v, 0, bytes, s));
    if (m->opt_aux) DCV_CHECK_HIP(hipMemsetAsync(m->opt_aux, 0, bytes, s));
    if (m->desc.optimizer == DCV_OPT_ADAGRAD && m->desc.initial_accumulator_value != 0.0) {
        hipLaunchKernelGGL(fill_kernel, dim3(256), dim3(256), 0, s, m->adam_v, m->n_params, (float)m->desc.initial_accumulator_value);
        DCV_CHECK_LAUNCH();
    }
    // Rprop's step_size and ASGD's eta are created by torch inside the FIRST optimizer.step(), from the learning rate the
    // group holds at that moment -- after a scheduler's constructor (OneCycleLR, LinearLR, a warm-up LambdaLR) has already
    // rescaled it: seeded in first_step_state(), right before the first update, from m->lr
    m->nadam_mu_product = 1.0;
    m->asgd_eta = (double)(float)m->lr;
    m->adam_t = 0;
    m->drop_step = 0;
    return DCV_OK;
}

// What one reduction folds: the layers [l0, l1) of `ra_all` and the batch normalisations behind them, with the extents that
// pick its kernel.
struct ReduceSet {
    ReduceArgs ra;
    int max_splits = 0, max_bblocks = 0;
    int64_t max_total = 0;
};
static ReduceSet reduce_set(const dcv_mlp* m, const ReduceArgs& ra_all, int l0, int l1) {
    ReduceSet rs;
    rs.ra.L = 0;
    auto take = [&](const ReduceDesc& d) {
        rs.ra.l[rs.ra.L++] = d;
        if (d.splits > rs.max_splits) rs.max_splits = d.splits;
        if (d.bblocks > rs.max_bblocks) rs.max_bblocks = d.bblocks;
        if (d.w_count + d.out > rs.max_total) rs.max_total = d.w_count + d.out;
    };
    for (int l = l0; l < l1; ++l) take(ra_all.l[l]);
    for (int l = l0; l < l1; ++l)
        if (m->layers[l].bn) take(ra_all.l[m->L + l]);   // weight / bias of the batch normalisation behind layer l
    return rs;
}
static bool quad_takes(const ReduceSet& rs) {
    static const bool quad_off = env_is("DCV_REDUCE_QUAD", '0');
    return rs.max_splits <= 512 && rs.max_bblocks <= 1024 && !quad_off;
}
// The items of the flat-grid reduction in the set's order (weights, then biases, of every entry).  part: 0 = all of them,
// 1 = the weights of entry 0 alone, 2 = everything but those (the split of a step whose upper gradients rode in the layer-0
// weight-gradient launch: ride_upper).
static int quad_items(const ReduceSet& rs, int part, QuadArgs* qa, int64_t* blocks_out) {
    qa->n = 0;
    int64_t blocks = 0;
    auto item = [&](const float* src, int64_t dst, int64_t count, int parts, int64_t stride) {
        if (count <= 0) return;
        if (!src || parts < 0) parts = 0;   // no partials: a zero gradient, as the other two kernels give
        QuadItem& q = qa->it[qa->n++];
        q = QuadItem{src, dst, stride, (int)count, parts, (int)blocks, quad_groups(parts)};
        blocks += cdiv(count, 1024 / q.groups);
    };
    for (int l = 0; l < rs.ra.L; ++l) {
        const ReduceDesc& d = rs.ra.l[l];
        DCV_REQUIRE(d.w_count < (1ll << 31), "reduce: layer too large");
        if (part == 0 || (part == 1) == (l == 0)) item(d.slab, d.w_off, d.w_count, d.splits, rd_wstride(d));
        if (part != 1) item(d.bpart, d.b_off, d.out, d.bblocks, rd_bstride(d));
    }
    DCV_REQUIRE(blocks < (1ll << 31), "reduce: grid out of range");
    *blocks_out = blocks;
    return DCV_OK;
}
static int launch_quad(dcv_mlp* m, const QuadArgs& qa, int64_t blocks, bool fuse_opt, const OptArgs& oa, hipStream_t s) {
    hipLaunchKernelGGL(reduce_grads_quad_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qa, m->grads, 1.f, fuse_opt ? 1 : 0, m->params, m->adam_m,
                       m->adam_v, m->opt_aux, oa);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

// Gradient reduction of the layers [l0, l1) of `ra` (split-K slabs + bias partials -> m->grads), optionally with the
// optimiser update fused in.
static int launch_reduce(dcv_mlp* m, const ReduceArgs& ra_all, int l0, int l1, bool fuse_opt, const OptArgs& oa, hipStream_t s) {
    const ReduceSet rs = reduce_set(m, ra_all, l0, l1);
    const ReduceArgs& ra = rs.ra;
    if (ra.L <= 0) return DCV_OK;
    if (quad_takes(rs)) {
        QuadArgs qa;
        int64_t blocks = 0;
        const int rc = quad_items(rs, 0, &qa, &blocks);
        if (rc) return rc;
        if (blocks <= 0) return DCV_OK;
        m->last_reduce = 1;
        return launch_quad(m, qa, blocks, fuse_opt, oa, s);
    } else if (rs.max_splits <= 512 && rs.max_bblocks <= 1024) {   // few partials per weight (the few bias elements may see more)
        int64_t bx = cdiv(rs.max_total, 64);
        if (bx > 2048) bx = 2048;
        m->last_reduce = 2;
        hipLaunchKernelGGL(reduce_grads_small_kernel, dim3((unsigned)bx, ra.L), dim3(256), 0, s, ra, m->grads, 1.f, fuse_opt ? 1 : 0, m->params,
                           m->adam_m, m->adam_v, m->opt_aux, oa);
    } else {
        m->last_reduce = 3;
        hipLaunchKernelGGL(reduce_grads_kernel, dim3(512, ra.L), dim3(64 * kRedWaves), 0, s, ra, m->grads, 1.f, fuse_opt ? 1 : 0, m->params, m->adam_m,
                           m->adam_v, m->opt_aux, oa);
    }
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}
int launch_reduce(dcv_mlp* m, const ReduceArgs& ra, int l0, int l1, hipStream_t s) { return launch_reduce(m, ra, l0, l1, false, OptArgs{}, s); }

// arguments of the next optimiser update; advances the step count
static OptArgs next_opt_args(dcv_mlp* m) {
    m->adam_t += 1;
    const dcv_mlp_desc& d = m->desc;
    const double t = (double)m->adam_t;
    OptArgs a{};   // (every scalar an optimiser does not use stays 0)
    a.kind = d.optimizer;
    a.first = m->adam_t == 1;
    a.lr = (float)m->lr;
    a.decay = 1.f;
    a.eps = (float)d.eps;
    a.wd = (float)d.weight_decay;
    a.maximize = d.maximize ? 1 : 0;
    a.img = m->snet_img;
    a.img_idx = m->snet_img_idx;
    switch (d.optimizer) {
        case DCV_OPT_ADAM:
        case DCV_OPT_ADAMW: {
            const double b1 = m->momentum_rt, b2 = d.beta2;   // beta1 may be cycled by a scheduler (dcv_mlp_set_momentum)
            a.flag = d.amsgrad ? 1 : 0;
            a.b1 = (float)b1;
            a.b2 = (float)b2;
            a.w1 = (float)(1.0 - b1);
            a.w2 = (float)(1.0 - b2);
            a.c1 = (float)(m->lr / (1.0 - pow(b1, t)));
            a.c2 = (float)sqrt(1.0 - pow(b2, t));
            a.decay = (float)(1.0 - m->lr * d.weight_decay);
            break;
        }
        case DCV_OPT_SGD:
            a.flag = d.nesterov ? 1 : 0;
            a.b1 = (float)m->momentum_rt;
            a.w1 = (float)(1.0 - d.dampening);
            break;
        case DCV_OPT_RMSPROP:
            a.flag = d.centered ? 1 : 0;
            a.b1 = (float)m->momentum_rt;
            a.b2 = (float)d.alpha;
            a.w2 = (float)(1.0 - d.alpha);
            break;
        case DCV_OPT_ADAMAX: {
            const double b1 = m->momentum_rt;
            a.b1 = (float)b1;
            a.b2 = (float)d.beta2;
            a.w1 = (float)(1.0 - b1);
            a.c1 = (float)(m->lr / (1.0 - pow(b1, t)));
            break;
        }
        case DCV_OPT_NADAM: {
            const double b1 = m->momentum_rt, b2 = d.beta2, md = d.opt_p[0];
            a.flag = d.opt_p[1] != 0.0 ? 1 : 0;
            a.b1 = (float)b1;
            a.b2 = (float)b2;
            a.w1 = (float)(1.0 - b1);
            a.w2 = (float)(1.0 - b2);
            a.c2 = (float)(1.0 - pow(b2, t));
            a.decay = (float)(1.0 - m->lr * d.weight_decay);
            const double mu = b1 * (1.0 - 0.5 * pow(0.96, t * md));
            const double mu_next = b1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * md));
            // the state tensor mu_product is float32: `mu_product *= mu`, then read back through .item()
            m->nadam_mu_product = (double)(float)((double)(float)m->nadam_mu_product * mu);
            const double mp = m->nadam_mu_product, mp_next = mp * mu_next;
            a.p0 = (float)(-m->lr * (1.0 - mu) / (1.0 - mp));
            a.p1 = (float)((-m->lr * mu_next) / (1.0 - mp_next));
            break;
        }
        case DCV_OPT_RADAM: {
            const double b1 = m->momentum_rt, b2 = d.beta2;
            a.flag = d.opt_p[1] != 0.0 ? 1 : 0;
            a.b1 = (float)b1;
            a.b2 = (float)b2;
            a.w1 = (float)(1.0 - b1);
            a.w2 = (float)(1.0 - b2);
            a.decay = (float)(1.0 - m->lr * d.weight_decay);
            const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
            a.c1 = (float)bc1;
            a.c2 = (float)sqrt(bc2);
            const double rho_inf = 2.0 / (1.0 - b2) - 1.0;
            const double rho_t = rho_inf - 2.0 * t * pow(b2, t) / bc2;
            a.p0 = rho_t > 5.0 ? (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)) : 0.f;
            break;
        }
        case DCV_OPT_ADADELTA:
            a.b2 = (float)d.opt_p[0];
            a.w2 = (float)(1.0 - d.opt_p[0]);
            break;
        case DCV_OPT_ASGD: {
            // eta is a float32 state tensor: written as lr / (1 + lambd lr step)^alpha after every step, read back through .item()
            const double eta = m->asgd_eta;
            a.p0 = (float)(1.0 - d.opt_p[0] * eta);
            a.p1 = (float)eta;
            m->asgd_eta = (double)(float)(m->lr / pow(1.0 + d.opt_p[0] * m->lr * t, d.opt_p[1]));
            break;
        }
        case DCV_OPT_RPROP:
            a.p0 = (float)d.opt_p[0];
            a.p1 = (float)d.opt_p[1];
            a.p2 = (float)d.opt_p[2];
            a.p3 = (float)d.opt_p[3];
            break;
        default:   // DCV_OPT_ADAGRAD
            a.c1 = (float)(m->lr / (1.0 + (t - 1.0) * d.lr_decay));
            break;
    }
    return a;
}

// state that torch.optim creates lazily in its first step(): called (with the stream of the update) before next_opt_args
static int first_step_state(dcv_mlp* m, hipStream_t s) {
    if (m->adam_t != 0) return DCV_OK;
    if (m->desc.optimizer == DCV_OPT_RPROP) {   // step_size = full_like(grad, lr)
        hipLaunchKernelGGL(fill_kernel, dim3(256), dim3(256), 0, s, m->adam_v, m->n_params, (float)m->lr);
        DCV_CHECK_LAUNCH();
    }
    if (m->desc.optimizer == DCV_OPT_ASGD) m->asgd_eta = (double)(float)m->lr;   // eta = as_tensor(lr)
    return DCV_OK;
}

ReduceArgs reduce_args_of(const dcv_mlp* m, const ReduceArgsView& v) {
    ReduceArgs ra{};
    ra.L = m->L;
    for (int l = 0; l < m->L; ++l) {
        ReduceDesc& rd = ra.l[l];
        rd = linear_reduce_desc(m->layers[l], v.splits[l], v.bblocks[l]);
        rd.slab = v.slab[l];
        rd.bpart = v.bpart[l];
        rd.w_stride = v.wstride[l];
        rd.b_stride = v.bstride[l];
    }
    return ra;
}
// Data-parallel overlap hook (dcv_mlp_set_upper_grads_callback): the gradients of layers [1, L) are reduced on their own and
// the caller is told, once per backward (*done) and never when the optimiser is fused into the reduction.
int reduce_upper(dcv_mlp* m, const ReduceArgs& ra, bool fuse_opt, bool* done, hipStream_t s) {
    if (*done || m->L <= 1 || !m->upper_cb || fuse_opt) return DCV_OK;
    const int rc = launch_reduce(m, ra, 1, m->L, s);
    if (rc) return rc;
    *done = true;
    m->upper_cb(m->upper_cb_user);
    return DCV_OK;
}
// One-GPU training step with the update fused in (no upper-gradients callback, L >= 2, the flat-grid reduction): the layer-0
// weight gradient is the last product of the backward and the only one the gradients of W0 wait for.  Every other item of
// the final reduction -- the weights of layers 1 .. L-1, every bias (layer 0's fell out of the input gradient of layer 1), the
// batch normalisations -- has its partials complete before that product starts and is read by nothing in it, so those
// items are reduced and updated by extra workgroups of ITS launch (ride.hip); the final launch then holds the W0 item alone.
// Items, their order among themselves, the arithmetic and the update's arguments are those of the single reduction: the
// arguments are formed here, once (the step count advances here), and handed on to finish_grads through *oa.
// Returns 1 when it does not apply (nothing was launched, no state was touched: the caller launches the product alone).
int ride_upper(dcv_mlp* m, const ReduceArgs& ra, const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t k_chunk,
               const EpiSlab& epi, OptArgs* oa, hipStream_t s) {
    static const bool off = env_is("DCV_NO_REDUCE_RIDE", '1');
    if (off || m->upper_cb || m->L < 2) return 1;
    const ReduceSet rs = reduce_set(m, ra, 0, m->L);
    if (!quad_takes(rs) || !wgrad_reduce_applies(A, B, M, N, K, k_chunk)) return 1;
    QuadArgs qa;
    int64_t blocks = 0;
    int rc = quad_items(rs, 2, &qa, &blocks);
    if (rc) return rc;
    if (blocks <= 0) return 1;
    rc = first_step_state(m, s);
    if (rc) return rc;
    *oa = next_opt_args(m);
    rc = launch_wgrad_reduce(A, B, M, N, K, k_chunk, epi, qa, blocks, m->grads, m->params, m->adam_m, m->adam_v, m->opt_aux, *oa, s);
    if (rc) return rc;
    m->last_ride = (int)blocks;
    return DCV_OK;
}
// The end of every backward: the upper layers' early reduction unless it went out already, the arguments of the fused
// update (which advance the optimiser's host state: run_graphed snapshots it around this), the final reduction.
// ridden: the update's arguments when ride_upper took everything but the weights of layer 0 (and advanced the state).
int finish_grads(dcv_mlp* m, const ReduceArgs& ra, bool fuse_opt, bool upper_done, hipStream_t s, const OptArgs* ridden) {
    if (ridden) {
        QuadArgs qa;
        int64_t blocks = 0;
        const int rcq = quad_items(reduce_set(m, ra, 0, m->L), 1, &qa, &blocks);
        if (rcq || blocks <= 0) return rcq;
        m->last_reduce = 1;
        return launch_quad(m, qa, blocks, true, *ridden, s);
    }
    int rc = reduce_upper(m, ra, fuse_opt, &upper_done, s);
    if (rc) return rc;
    OptArgs oa{};
    if (fuse_opt) {
        rc = first_step_state(m, s);
        if (rc) return rc;
        oa = next_opt_args(m);
    }
    return launch_reduce(m, ra, 0, upper_done ? 1 : m->L, fuse_opt, oa, s);   // layer 0 only when the upper layers went out early
}
int apply_impl(dcv_mlp* m, void* stream) {
    DCV_REQUIRE(m, "dcv_mlp_apply: null");
    hipStream_t s = as_stream(stream);
    const int rcf = first_step_state(m, s);
    if (rcf) return rcf;
    const OptArgs a = next_opt_args(m);
    int64_t blocks = cdiv(m->n_params, 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(optimizer_kernel, dim3((unsigned)blocks), dim3(256), 0, s, m->params, (const float*)m->grads, m->adam_m, m->adam_v,
                       m->opt_aux, m->n_params, a);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

}  // namespace dcv

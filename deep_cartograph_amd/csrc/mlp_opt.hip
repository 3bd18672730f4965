// MLP engine, optimiser unit: the torch.optim single-tensor updates and the ordered reduction of the gradient partials
// (split-K weight slabs, bias column sums) that ends every backward pass -- on one GPU with the update fused in.
#include "mlp_state.h"
#include <math.h>

namespace dcv {

static inline int64_t rd_wstride(const ReduceDesc& d) { return d.w_stride > 0 ? d.w_stride : d.w_count; }
static inline int64_t rd_bstride(const ReduceDesc& d) { return d.b_stride > 0 ? d.b_stride : (int64_t)d.out; }

// torch.optim single-tensor updates (CPU code path of torch 2.x: _single_tensor_adam / _adamw / _sgd / _rmsprop /
// _adagrad), fp32 state.  One thread per element; `s1`, `s2`, `s3` are the optimiser's state tensors.
struct OptArgs {
    int kind, flag;   // DCV_OPT_*; flag: amsgrad (Adam family), nesterov (SGD), centered (RMSprop)
    int first;        // SGD: first step (momentum buffer := gradient)
    float lr, b1, b2, eps, wd;
    float c1, c2;     // Adam family: lr / (1 - b1^t), sqrt(1 - b2^t); Adagrad: c1 = lr / (1 + (t - 1) lr_decay)
    // scalars torch forms in Python doubles and then hands to a float32 kernel: computed on the host in double and
    // rounded once, exactly as there ((float)(1 - 0.999) is not 1.f - 0.999f)
    float w1, w2;     // 1 - beta1 (Adam) / 1 - dampening (SGD) ; 1 - beta2 (Adam) / 1 - alpha (RMSprop)
    float decay;      // AdamW: 1 - lr * weight_decay
    float p0, p1, p2, p3;   // further per-step scalars of Adamax / NAdam / RAdam / Adadelta / ASGD / Rprop (next_opt_args)
    int maximize;           // torch.optim's maximize: the update runs on the negated gradient
    // LDS image of the fused small-network kernels (snet.h: snet_image_build): every updated parameter is mirrored into the
    // zero-padded weight image those kernels stage with one contiguous copy, at img[img_idx[i]] (img_idx[i] < 0: not in it)
    float* img;
    const int* img_idx;
};
// pi = p[i], loaded by the caller (the reduction kernels issue that load before they wait for the partial sums)
// WT: write-through stores (the launch then ends without dirty lines to write back: reduce_grads_quad_kernel)
template <bool WT>
__device__ __forceinline__ void opt_st(float* p, float v) {
    if constexpr (WT) handoff_store(p, v);
    else *p = v;
}
template <bool WT>
__device__ __forceinline__ void opt_stp(const OptArgs& a, float* p, int64_t i, float v) {
    opt_st<WT>(p + i, v);
    if (a.img != nullptr) {
        const int j = a.img_idx[i];
        if (j >= 0) opt_st<WT>(a.img + j, v);
    }
}
template <bool WT = false>
__device__ __forceinline__ void opt_update_p(int64_t i, float gi, float pi, float* __restrict__ p, float* __restrict__ s1, float* __restrict__ s2,
                                             float* __restrict__ s3, const OptArgs& a) {
    if (a.maximize) gi = -gi;   // `grad = grads[i] if not maximize else -grads[i]`: the first line of every _single_tensor_* update
    switch (a.kind) {
        case DCV_OPT_ADAM:
        case DCV_OPT_ADAMW: {
            if (a.kind == DCV_OPT_ADAMW) pi = pi * a.decay;                        // param.mul_(1 - lr * weight_decay)
            else if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);                        // grad.add(param, alpha=weight_decay)
            float mi = s1[i], vi = s2[i];
            mi = mi + (gi - mi) * a.w1;                                           // exp_avg.lerp_(grad, 1 - beta1)
            vi = vi * a.b2 + a.w2 * gi * gi;                                      // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            float vden = vi;
            if (a.flag) {                                                          // amsgrad: max_exp_avg_sq = max(., exp_avg_sq)
                vden = fmaxf(s3[i], vi);
                opt_st<WT>(s3 + i, vden);
            }
            const float denom = sqrtf(vden) / a.c2 + a.eps;
            opt_st<WT>(s1 + i, mi);
            opt_st<WT>(s2 + i, vi);
            opt_stp<WT>(a, p, i, pi - a.c1 * (mi / denom));                                      // param.addcdiv_(exp_avg, denom, value=-step_size)
            break;
        }
        case DCV_OPT_SGD: {
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            if (a.b1 != 0.f) {                                                     // b1 = momentum, w1 = 1 - dampening
                float bi = a.first ? gi : s1[i] * a.b1 + a.w1 * gi;               // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
                opt_st<WT>(s1 + i, bi);
                gi = a.flag ? fmaf(a.b1, bi, gi) : bi;                            // nesterov: grad.add(buf, alpha=momentum)
            }
            opt_stp<WT>(a, p, i, pi - a.lr * gi);
            break;
        }
        case DCV_OPT_RMSPROP: {
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            float sq = s2[i] * a.b2 + a.w2 * gi * gi;                             // square_avg.mul_(alpha).addcmul_(grad, grad, 1 - alpha)
            opt_st<WT>(s2 + i, sq);
            float avg;
            if (a.flag) {                                                          // centered
                float ga = s3[i];
                ga = ga + (gi - ga) * a.w2;                                        // grad_avg.lerp_(grad, 1 - alpha)
                opt_st<WT>(s3 + i, ga);
                avg = sqrtf(sq - ga * ga) + a.eps;                                 // addcmul(grad_avg, grad_avg, -1).sqrt_().add_(eps)
            } else {
                avg = sqrtf(sq) + a.eps;
            }
            if (a.b1 > 0.f) {                                                      // b1 = momentum
                const float bi = s1[i] * a.b1 + gi / avg;                          // buf.mul_(momentum).addcdiv_(grad, avg)
                opt_st<WT>(s1 + i, bi);
                opt_stp<WT>(a, p, i, pi - a.lr * bi);
            } else {
                opt_stp<WT>(a, p, i, pi - a.lr * (gi / avg));
            }
            break;
        }
        case DCV_OPT_ADAMAX: {   // _single_tensor_adamax: s1 = exp_avg, s2 = exp_inf
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            float mi = s1[i];
            mi = mi + (gi - mi) * a.w1;                                           // exp_avg.lerp_(grad, 1 - beta1)
            const float ui = fmaxf(s2[i] * a.b2, fabsf(gi) + a.eps);              // maximum(exp_inf * beta2, |grad| + eps)
            opt_st<WT>(s1 + i, mi);
            opt_st<WT>(s2 + i, ui);
            opt_stp<WT>(a, p, i, pi - a.c1 * (mi / ui));                                         // addcdiv_(exp_avg, exp_inf, value=-lr / bias_correction)
            break;
        }
        case DCV_OPT_NADAM: {    // _single_tensor_nadam: p0 = -lr (1 - mu) / (1 - mu_product), p1 = -lr mu_next / (1 - mu_product_next), c2 = 1 - beta2^t
            if (a.wd != 0.f) {
                if (a.flag) pi = pi * a.decay;                                     // decoupled: param.mul_(1 - lr * weight_decay)
                else gi = fmaf(a.wd, pi, gi);
            }
            float mi = s1[i], vi = s2[i];
            mi = mi + (gi - mi) * a.w1;
            vi = vi * a.b2 + a.w2 * gi * gi;
            const float denom = sqrtf(vi / a.c2) + a.eps;                          // exp_avg_sq.div(bias_correction2).sqrt().add(eps)
            opt_st<WT>(s1 + i, mi);
            opt_st<WT>(s2 + i, vi);
            pi = pi + a.p0 * (gi / denom);
            opt_stp<WT>(a, p, i, pi + a.p1 * (mi / denom));
            break;
        }
        case DCV_OPT_RADAM: {    // _single_tensor_radam: c1 = 1 - beta1^t, c2 = sqrt(1 - beta2^t), p0 = rect (0: rho_t <= 5)
            if (a.wd != 0.f) {
                if (a.flag) pi = pi * a.decay;
                else gi = fmaf(a.wd, pi, gi);
            }
            float mi = s1[i], vi = s2[i];
            mi = mi + (gi - mi) * a.w1;
            vi = vi * a.b2 + a.w2 * gi * gi;
            opt_st<WT>(s1 + i, mi);
            opt_st<WT>(s2 + i, vi);
            const float mhat = mi / a.c1;
            if (a.p0 > 0.f) opt_stp<WT>(a, p, i, pi - ((mhat * a.lr) * (a.c2 / (sqrtf(vi) + a.eps))) * a.p0);
            else opt_stp<WT>(a, p, i, pi - mhat * a.lr);
            break;
        }
        case DCV_OPT_ADADELTA: { // _single_tensor_adadelta: s1 = square_avg, s2 = acc_delta, b2 = rho, w2 = 1 - rho
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            const float sq = s1[i] * a.b2 + a.w2 * gi * gi;
            const float acc = s2[i];
            const float delta = sqrtf(acc + a.eps) / sqrtf(sq + a.eps) * gi;
            opt_st<WT>(s1 + i, sq);
            opt_st<WT>(s2 + i, acc * a.b2 + a.w2 * delta * delta);
            opt_stp<WT>(a, p, i, pi - a.lr * delta);
            break;
        }
        case DCV_OPT_ASGD: {     // _single_tensor_asgd: p0 = 1 - lambd * eta, p1 = eta (the averaged copy ax is not kept)
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            pi = pi * a.p0;
            opt_stp<WT>(a, p, i, pi - a.p1 * gi);
            break;
        }
        case DCV_OPT_RPROP: {    // _single_tensor_rprop: s1 = prev, s2 = step_size; p0 / p1 = eta minus / plus, p2 / p3 = step bounds
            const float sg = gi * s1[i];
            const float f = sg > 0.f ? a.p1 : (sg < 0.f ? a.p0 : 1.f);
            const float st = fminf(fmaxf(s2[i] * f, a.p2), a.p3);
            opt_st<WT>(s2 + i, st);
            if (sg < 0.f) gi = 0.f;
            const float sgn = gi > 0.f ? 1.f : (gi < 0.f ? -1.f : 0.f);
            opt_stp<WT>(a, p, i, pi - sgn * st);
            opt_st<WT>(s1 + i, gi);
            break;
        }
        default: {   // DCV_OPT_ADAGRAD
            if (a.wd != 0.f) gi = fmaf(a.wd, pi, gi);
            const float su = s2[i] + gi * gi;                                      // state_sum.addcmul_(grad, grad, value=1)
            opt_st<WT>(s2 + i, su);
            opt_stp<WT>(a, p, i, pi - a.c1 * (gi / (sqrtf(su) + a.eps)));                         // param.addcdiv_(grad, std, value=-clr)
            break;
        }
    }
}
__device__ __forceinline__ void opt_update(int64_t i, float gi, float* __restrict__ p, float* __restrict__ s1, float* __restrict__ s2,
                                           float* __restrict__ s3, const OptArgs& a) {
    opt_update_p(i, gi, p[i], p, s1, s2, s3, a);
}
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

// The small-split reduction on a flat grid with 16-byte loads.  The weights and the biases of every entry are separate
// items {partials, count, number of partials}; the grid is the concatenation of the items' blocks (no empty workgroups
// for the narrow layers).  A block of 256 threads covers 1024 / G consecutive elements with G groups of threads, group g
// taking the partials q = g, g + G, ... (four consecutive elements per thread: one global_load_dwordx4 per partial
// where the item allows); G = 4 for few partials, 16 when an item has more than 32 (the 129 bias partials of the
// 64-row tiles, the 257 of the fused last-layer pass: walked by 4 groups they are a chain of 64 dependent-latency
// loads, the longest path of the launch).  After the exchange every thread of the first 1024 / G finishes ONE element,
// groups combined in order, float64: deterministic -- and its parameter load was issued before the partials were
// waited for.
struct QuadItem {
    const float* src;   // [parts][stride], count <= stride values used
    int64_t dst;        // offset of element 0 in grads / params
    int64_t stride;     // floats between partials
    int count, parts;
    int blk0;           // first block of this item in the grid
    int groups;         // G
};
struct QuadArgs {
    QuadItem it[4 * DCV_MAX_LAYERS];
    int n;
};
inline int quad_groups(int parts) { return parts > 32 ? 16 : 4; }
template <int G>
__device__ __forceinline__ void reduce_quad_block(const QuadItem& d, int blk, float* __restrict__ grads, float scale, int fuse,
                                                  float* __restrict__ params, float* __restrict__ s1, float* __restrict__ s2,
                                                  float* __restrict__ s3, const OptArgs& oa, double* s_red) {
    constexpr int EPB = 1024 / G, TPG = EPB / 4;   // elements per block, threads per group
    const int t = threadIdx.x, g = t / TPG, sub = t % TPG;
    const int base = blk * EPB;
    const int mine = base + t;
    const bool fin = t < EPB && mine < d.count;
    float pi = 0.f;
    if (fuse && fin) pi = params[d.dst + mine];
    const int e0 = base + 4 * sub;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (e0 < d.count && (d.stride & 3) == 0 && e0 + 4 <= d.stride && (reinterpret_cast<uintptr_t>(d.src) & 15) == 0) {
        // (the last quad of a partial may reach into its padding: those elements are summed and never finished)
        const float* p = d.src + e0;
#pragma unroll 8
        for (int q = g; q < d.parts; q += G) {
            const float4 v = *reinterpret_cast<const float4*>(p + (int64_t)q * d.stride);
            acc[0] += (double)v.x;
            acc[1] += (double)v.y;
            acc[2] += (double)v.z;
            acc[3] += (double)v.w;
        }
    } else if (e0 < d.count) {
        const float* p = d.src + e0;
        const int nv = d.count - e0 < 4 ? d.count - e0 : 4;
#pragma unroll 4
        for (int q = g; q < d.parts; q += G) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) acc[j] += (double)p[(int64_t)q * d.stride + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s_red[g * EPB + 4 * sub + j] = acc[j];
    __syncthreads();
    if (fin) {
        double tot = s_red[t];
#pragma unroll
        for (int k = 1; k < G; ++k) tot += s_red[k * EPB + t];
        const float gr = (float)(tot * (double)scale);
        handoff_store(grads + d.dst + mine, gr);
        if (fuse) opt_update_p<true>(d.dst + mine, gr, pi, params, s1, s2, s3, oa);
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

// Gradient reduction of the layers [l0, l1) of `ra` (split-K slabs + bias partials -> m->grads), optionally with the
// optimiser update fused in.
static int launch_reduce(dcv_mlp* m, const ReduceArgs& ra_all, int l0, int l1, bool fuse_opt, const OptArgs& oa, hipStream_t s) {
    ReduceArgs ra;
    ra.L = 0;
    int max_splits = 0, max_bblocks = 0;
    int64_t max_total = 0;
    auto take = [&](const ReduceDesc& d) {
        ra.l[ra.L++] = d;
        if (d.splits > max_splits) max_splits = d.splits;
        if (d.bblocks > max_bblocks) max_bblocks = d.bblocks;
        if (d.w_count + d.out > max_total) max_total = d.w_count + d.out;
    };
    for (int l = l0; l < l1; ++l) take(ra_all.l[l]);
    for (int l = l0; l < l1; ++l)
        if (m->layers[l].bn) take(ra_all.l[m->L + l]);   // weight / bias of the batch normalisation behind layer l
    if (ra.L <= 0) return DCV_OK;
    static const bool quad_off = [] { const char* e = getenv("DCV_REDUCE_QUAD"); return e && e[0] == '0'; }();
    if (max_splits <= 512 && max_bblocks <= 1024 && !quad_off) {
        QuadArgs qa;
        qa.n = 0;
        int64_t blocks = 0;
        auto item = [&](const float* src, int64_t dst, int64_t count, int parts, int64_t stride) {
            if (count <= 0) return;
            if (!src || parts < 0) parts = 0;   // no partials: a zero gradient, as the other two kernels give
            QuadItem& q = qa.it[qa.n++];
            q = QuadItem{src, dst, stride, (int)count, parts, (int)blocks, quad_groups(parts)};
            blocks += cdiv(count, 1024 / q.groups);
        };
        for (int l = 0; l < ra.L; ++l) {
            DCV_REQUIRE(ra.l[l].w_count < (1ll << 31), "reduce: layer too large");
            item(ra.l[l].slab, ra.l[l].w_off, ra.l[l].w_count, ra.l[l].splits, rd_wstride(ra.l[l]));
            item(ra.l[l].bpart, ra.l[l].b_off, ra.l[l].out, ra.l[l].bblocks, rd_bstride(ra.l[l]));
        }
        if (blocks <= 0) return DCV_OK;
        DCV_REQUIRE(blocks < (1ll << 31), "reduce: grid out of range");
        hipLaunchKernelGGL(reduce_grads_quad_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qa, m->grads, 1.f, fuse_opt ? 1 : 0, m->params,
                           m->adam_m, m->adam_v, m->opt_aux, oa);
    } else if (max_splits <= 512 && max_bblocks <= 1024) {   // few partials per weight (the few bias elements may see more)
        int64_t bx = cdiv(max_total, 64);
        if (bx > 2048) bx = 2048;
        hipLaunchKernelGGL(reduce_grads_small_kernel, dim3((unsigned)bx, ra.L), dim3(256), 0, s, ra, m->grads, 1.f, fuse_opt ? 1 : 0, m->params,
                           m->adam_m, m->adam_v, m->opt_aux, oa);
    } else {
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
// The end of every backward: the upper layers' early reduction unless it went out already, the arguments of the fused
// update (which advance the optimiser's host state: run_graphed snapshots it around this), the final reduction.
int finish_grads(dcv_mlp* m, const ReduceArgs& ra, bool fuse_opt, bool upper_done, hipStream_t s) {
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

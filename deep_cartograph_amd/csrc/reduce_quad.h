// The optimiser update and the flat-grid ("quad") reduction block: shared by the reduction launch (mlp_opt.hip) and the launch
// that carries reduction blocks beside the layer-0 weight gradient (ride.hip).
#pragma once
#include "gemm_kernels.h"
#include "handoff.h"

namespace dcv {

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

// ride.hip: the layer-0 weight gradient (gemm_tn_slab's product) with `qblocks` reduction blocks of `qa` behind its workgroups, update fused
bool wgrad_reduce_applies(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t k_chunk);
int launch_wgrad_reduce(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t k_chunk, const EpiSlab& e, const QuadArgs& qa,
                        int64_t qblocks, float* grads, float* params, float* s1, float* s2, float* s3, const OptArgs& oa, hipStream_t s);

}  // namespace dcv

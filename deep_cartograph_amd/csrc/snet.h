// Pieces shared by the fused small-network kernels (snet.hip: autoencoder step; snet_dt.hip: Deep-TICA forward / backward):
// the LDS layout of the zero-padded weight images, the v_mfma_f32_16x16x4_f32 tile products with compile-time contraction
// lengths, the activation helpers; every phase the kernels have in common (weight staging, forward layer, input / weight /
// bias gradient of a layer) and the host code their plans share (activation map, partials layout, launch).  What is specific
// to a model stays in its unit.  See snet.hip for the design notes.
#pragma once
#include <hip/hip_ext.h>
#include "mlp_state.h"
#include <type_traits>
#include <vector>

namespace dcv {

typedef float sv4f __attribute__((ext_vector_type(4)));

constexpr int kSnetThreads = 512;   // 8 waves: two per SIMD, one hides the other's LDS and MFMA latency
constexpr int kSnetWaves = kSnetThreads / 64;

struct SnetLayer {
    int in, out, pin, pout, act;
    int nk_in, nk_out;          // pin / 16, pout / 16
    int u4_begin, c4_shift;     // staging: first 16-byte unit of this layer's weight image in the flat unit space; log2(pin / 4)
    int64_t w_off, b_off;       // flat parameter buffer
    int lw, lb, pws;            // LDS float offsets of the weight image [pout][pws] and the bias [pout]; pws = pin + 4
    int64_t pw_off, pb_off;     // gradient partials: part + pw_off + wg * pw_stride ; part + pb_off + wg * pb_stride
    int pw_stride, pb_stride;   // out * in and out rounded up to multiples of 4 floats (16-byte loads in the reduction)
};
__device__ __forceinline__ sv4f mfma4(float a, float b, sv4f c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Contraction lengths are compile-time (NK chunks of 16; the plan pads every width to 16 * 2^j): the fragment reads of
// a tile are issued back to back, the MFMAs run in up to four independent accumulator chains, no branch in between.
// (With run-time trip counts hipcc emitted ds_read -> s_waitcnt lgkmcnt(0) -> 4 dependent MFMAs -> branch per chunk:
// 1.2 us of fixed cost per layer, 51 us per fused step.)
template <int NK>
struct SnetFrags {
    sv4f f[NK];
    __device__ __forceinline__ void load(const float* p) {   // p: this lane's row, offset 4 * q; chunk j at p + 16 j
#pragma unroll
        for (int j = 0; j < NK; ++j) f[j] = *reinterpret_cast<const sv4f*>(p + 16 * j);
    }
};
template <int NK>
__device__ __forceinline__ sv4f snet_chain_sum(sv4f (&acc)[(NK < 4 ? NK : 4)]) {
    constexpr int C = NK < 4 ? NK : 4;
    sv4f r = acc[0];
#pragma unroll
    for (int c = 1; c < C; ++c) r += acc[c];
    return r;
}
// D[r][c] = sum_k A[r][k] W[c][k]  (forward: A = activations of the wave's 16 rows, W row-major [out][in])
template <int NK>
__device__ __forceinline__ sv4f snet_fwd_tile(const SnetFrags<NK>& A, const float* bp) {
    constexpr int C = NK < 4 ? NK : 4;
    SnetFrags<NK> B;
    B.load(bp);
    sv4f acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = sv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NK; ++j) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[j % C] = mfma4(A.f[j][s], B.f[j][s], acc[j % C]);
    }
    return snet_chain_sum<NK>(acc);
}
// D[r][i] = sum_o dZ[r][o] W[o][i]  (input gradient: A = dZ rows, B = a column block of W read down the rows)
template <int NK>
__device__ __forceinline__ sv4f snet_dgrad_tile(const SnetFrags<NK>& A, const float* bp, int pws) {
    constexpr int C = NK < 4 ? NK : 4;
    float b[NK][4];
#pragma unroll
    for (int j = 0; j < NK; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) b[j][s] = bp[(16 * j + s) * pws];
    sv4f acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = sv4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NK; ++j) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[j % C] = mfma4(A.f[j][s], b[j][s], acc[j % C]);
    }
    return snet_chain_sum<NK>(acc);
}
// D[o][i] = sum_r dZ[r][o] Hin[r][i], r < TR  (weight gradient of the tile)
template <int TR>
__device__ __forceinline__ sv4f snet_wgrad_tile(const float* ap, int psz, const float* bp, int psh) {
    float av[TR / 4], bv[TR / 4];
#pragma unroll
    for (int s = 0; s < TR / 4; ++s) {
        av[s] = ap[4 * s * psz];
        bv[s] = bp[4 * s * psh];
    }
    sv4f acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < TR / 4; s += 2) {
        acc0 = mfma4(av[s], bv[s], acc0);
        acc1 = mfma4(av[s + 1], bv[s + 1], acc1);
    }
    return acc0 + acc1;
}

// activation with the switch outside the element loop
__device__ __forceinline__ sv4f snet_act4(int act, sv4f z) {
    sv4f h;
    switch (act) {
        case DCV_ACT_NONE: h = z; break;
        case DCV_ACT_LEAKY_RELU:
#pragma unroll
            for (int v = 0; v < 4; ++v) h[v] = z[v] > 0.f ? z[v] : 0.01f * z[v];
            break;
        case DCV_ACT_RELU:
#pragma unroll
            for (int v = 0; v < 4; ++v) h[v] = z[v] > 0.f ? z[v] : 0.f;
            break;
        default:
#pragma unroll
            for (int v = 0; v < 4; ++v) h[v] = act_fwd(act, z[v]);
            break;
    }
    return h;
}
__device__ __forceinline__ sv4f snet_actgrad4(int act, sv4f h) {
    sv4f g;
    switch (act) {
        case DCV_ACT_NONE: g = sv4f{1.f, 1.f, 1.f, 1.f}; break;
        case DCV_ACT_LEAKY_RELU:
#pragma unroll
            for (int v = 0; v < 4; ++v) g[v] = h[v] > 0.f ? 1.f : 0.01f;
            break;
        case DCV_ACT_RELU:
#pragma unroll
            for (int v = 0; v < 4; ++v) g[v] = h[v] > 0.f ? 1.f : 0.f;
            break;
        default:
#pragma unroll
            for (int v = 0; v < 4; ++v) g[v] = act_grad_from_out(act, h[v]);
            break;
    }
    return g;
}

constexpr int kSnetMaxTiles = 8;   // column tiles of a layer per wave (input gradients are held in registers across a barrier)

// nk (chunks of 16 of a padded width: 1, 2, 4, 8 or 16) as a compile-time constant: f(std::integral_constant<int, NK>)
template <class F>
__device__ __forceinline__ void snet_nk_switch(int nk, F&& f) {
    switch (nk) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

// The kernel arguments are 2 KB (one table entry per layer and phase): touch every 64-byte line with a scalar load at the
// kernel's start, so that the first use of a layer's entry in the forward chain is a scalar-cache hit (measured with the
// new wave map: 21.2 -> 19.8 us per evaluation step, 48.2 -> 46.7 per training step on the same box).  The caller keeps
// the result alive up to the end of its staging: asm volatile("" ::"s"(x)).
template <int BYTES>
__device__ __forceinline__ unsigned snet_touch_kernargs() {
    unsigned x = 0;
    const __attribute__((address_space(4))) unsigned* kp = (const __attribute__((address_space(4))) unsigned*)__builtin_amdgcn_kernarg_segment_ptr();
#pragma unroll
    for (int off = 0; off < BYTES; off += 64) x ^= kp[off / 4];
    return x;
}

// A thread's place in a workgroup that works on a TR-row tile.  A wave owns a 16-row group and every CG-th column tile:
// wave -> (row group, column group) with consecutive waves (= the four SIMDs) on different column groups first, so a narrow
// layer with one or two column tiles keeps one wave on each SIMD instead of two waves on half of them.
template <int TR>
struct SnetCoords {
    static constexpr int RG = TR / 16, CG = kSnetWaves / RG;
    int t, lane, wave, rg, cg, q, n;
    __device__ __forceinline__ SnetCoords()
        : t(threadIdx.x), lane(t & 63), wave(t >> 6), rg(wave % RG), cg(wave / RG), q(lane >> 4), n(lane & 15) {}
};

// Table-driven staging of the entries [first, n) of the plan's staging table (snet_layout) into LDS, zero padding included:
// one flat space of 16-byte units over all layers, twelve independent loads in flight per thread and pass.  The table entries
// of pass p + 1 are requested behind the data loads of pass p and arrive in the same round trip: one dependent round trip per
// pass (+ the first table read) instead of two (round 4: 8 -> 5 for the C2 network's four passes).  Per-layer loops cost one
// L2 round trip per pass (8-11 us).
// hook(): the caller's ride-along loads, called in EVERY pass (the caller keeps its own "issued" flag) -- ahead of the pass's
// data loads (HOOK_FIRST: loads return in order, so what must not wait for the data goes first) or behind them (issued
// earlier, cold rows of X would hold up the table entries; behind, they ride along the data round trip).  Only the lanes with
// an entry left take the last pass: nothing wave-wide belongs in the hook.
template <int NT, bool HOOK_FIRST, class Hook>
__device__ __forceinline__ void snet_stage_table(const int2* tab, int first, int n, const float* params, float* sl, int t, Hook&& hook) {
    int2 e[12];
#pragma unroll
    for (int u = 0; u < 12; ++u) {
        const int i = first + t + NT * u;
        e[u] = i < n ? tab[i] : make_int2(-1, -1);
    }
    for (int i0 = first + t; i0 < n; i0 += 12 * NT) {
        float4 v[12];
        if (HOOK_FIRST) hook();
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e[u].x >= 0) {
                const float* src = params + e[u].x;
                const int nv = (e[u].y >> 20) & 7;
                if ((e[u].y >> 24) & 1) {
                    v[u] = *reinterpret_cast<const float4*>(src);
                } else {
                    v[u].x = src[0];
                    if (nv > 1) v[u].y = src[1];
                    if (nv > 2) v[u].z = src[2];
                    if (nv > 3) v[u].w = src[3];
                }
            }
        }
        if (!HOOK_FIRST) hook();
        int2 en[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) {
            const int i = i0 + 12 * NT + NT * u;
            en[u] = i < n ? tab[i] : make_int2(-1, -1);
        }
#pragma unroll
        for (int u = 0; u < 12; ++u)
            if (e[u].y >= 0) *reinterpret_cast<float4*>(sl + (e[u].y & 0xFFFFF)) = v[u];
#pragma unroll
        for (int u = 0; u < 12; ++u) e[u] = en[u];
    }
}

// Forward of one layer over the tile: Hout = act(Hin W^T + b), padding columns zero.  epilogue(h, col) sees this lane's four
// rows (rg * 16 + 4 q + v) of column col before they are stored (the autoencoder turns its last layer's output into dZ_L there).
template <int TR, class Epilogue>
__device__ __forceinline__ void snet_forward_layer(const SnetCoords<TR>& k, const SnetLayer& y, const float* sl, const float* Hin, int psin,
                                                   float* Hout, int pso, Epilogue&& epilogue) {
    const float* ap = Hin + (k.rg * 16 + k.n) * psin + 4 * k.q;
    const float* W = sl + y.lw + k.n * y.pws + 4 * k.q;
    snet_nk_switch(y.nk_in, [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        SnetFrags<NK> A;
        A.load(ap);
        for (int ct = k.cg; ct < y.nk_out; ct += SnetCoords<TR>::CG) {
            const sv4f acc = snet_fwd_tile<NK>(A, W + ct * 16 * y.pws);
            const int col = ct * 16 + k.n;
            const float bias = sl[y.lb + col];
            sv4f h = snet_act4(y.act, acc + bias);
            if (col >= y.out) h = sv4f{0.f, 0.f, 0.f, 0.f};
            epilogue(h, col);
#pragma unroll
            for (int v = 0; v < 4; ++v) Hout[(k.rg * 16 + 4 * k.q + v) * pso + col] = h[v];
        }
    });
}

// Input gradient of one layer, kept in registers: dg[j] = this wave's rows of dZ W, column tile cg + j * CG
template <int TR>
__device__ __forceinline__ void snet_dgrad_layer(const SnetCoords<TR>& k, const SnetLayer& y, const float* sl, const float* dZ, int psz,
                                                 sv4f (&dg)[kSnetMaxTiles]) {
    const float* ap = dZ + (k.rg * 16 + k.n) * psz + 4 * k.q;
    const float* W = sl + y.lw + (4 * k.q) * y.pws + k.n;
    snet_nk_switch(y.nk_out, [&](auto nk) {
        constexpr int NK = decltype(nk)::value;
        SnetFrags<NK> A;
        A.load(ap);
#pragma unroll
        for (int j = 0; j < kSnetMaxTiles; ++j) {
            const int it = k.cg + j * SnetCoords<TR>::CG;
            if (it < y.nk_in) dg[j] = snet_dgrad_tile<NK>(A, W + it * 16, y.pws);
        }
    });
}

// Weight gradient of the tile into this workgroup's partial: the nk_out x nk_in tiles round-robin over the waves.
// Hw [TR][psw]: the input of this Linear, dZ [TR][psz]: the gradient of its output.
template <int TR>
__device__ __forceinline__ void snet_wgrad_partials(const SnetCoords<TR>& k, const SnetLayer& y, float* part, const float* Hw, int psw,
                                                    const float* dZ, int psz) {
    const int nti = y.nk_in, ntot = y.nk_out * nti;
    float* pw = part + y.pw_off + (int64_t)blockIdx.x * y.pw_stride;
    const bool vec_ok = (y.in & 3) == 0 && ((y.pw_off + (int64_t)blockIdx.x * y.pw_stride) & 3) == 0;   // part is a hipMalloc base
    int ot = 0, it = k.wave;
    while (it >= nti) { it -= nti; ++ot; }
#pragma unroll 2
    for (int tile = k.wave; tile < ntot; tile += kSnetWaves) {
        // operands swapped (rows of the MFMA tile = input columns): a lane ends up with four CONSECUTIVE inputs
        // i of one output o = its 16 bytes of the partial's row -- one global_store_dwordx4 per tile and lane
        // instead of four 4-byte stores (the partial stores of the two wide layers were what these phases waited on)
        const sv4f acc = snet_wgrad_tile<TR>(Hw + k.q * psw + it * 16 + k.n, psw, dZ + k.q * psz + ot * 16 + k.n, psz);
        const int o = ot * 16 + k.n, i0 = it * 16 + 4 * k.q;
        if (o < y.out) {
            float* dst = pw + (int64_t)o * y.in + i0;
            if (vec_ok && i0 + 4 <= y.in) {
                handoff_store16(dst, acc);   // write-through: the 10 MB of partials are not left for the write-back at the launch's end (44.3 -> 42.8 us per step)
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (i0 + v < y.in) dst[v] = acc[v];
            }
        }
        it += kSnetWaves;
        while (it >= nti) { it -= nti; ++ot; }
    }
}
// Bias gradient into this workgroup's partial: column sums of dZ_l over the tile's rows, rows in index order
// (four threads per column, a quarter of the rows each, combined by two shuffles: a fixed order)
template <int TR>
__device__ __forceinline__ void snet_bgrad_partials(const SnetCoords<TR>& k, const SnetLayer& y, float* part, const float* dZ, int psz) {
    for (int o4 = k.t; o4 < 4 * y.pout; o4 += kSnetThreads) {
        const int o = o4 >> 2, quarter = o4 & 3;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < TR / 4; ++r) s += dZ[(quarter * (TR / 4) + r) * psz + o];
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (quarter == 0 && o < y.out) part[y.pb_off + (int64_t)blockIdx.x * y.pb_stride + o] = s;
    }
}

// dZ_{l-1} = dg * act'(H_l) written over H_l [TR][psh] (every wave is done reading it), zeros in the padding columns;
// y: layer l, act_prev / out_prev: activation and width of layer l - 1
template <int TR>
__device__ __forceinline__ void snet_dz_prev(const SnetCoords<TR>& k, const SnetLayer& y, int act_prev, int out_prev, float* Hin, int psh,
                                             const sv4f (&dg)[kSnetMaxTiles]) {
#pragma unroll
    for (int j = 0; j < kSnetMaxTiles; ++j) {
        const int it = k.cg + j * SnetCoords<TR>::CG;
        if (it < y.nk_in) {
            const int col = it * 16 + k.n;
            float* p = Hin + (k.rg * 16 + 4 * k.q) * psh + col;
            sv4f h;
#pragma unroll
            for (int v = 0; v < 4; ++v) h[v] = p[v * psh];
            const sv4f dh = snet_actgrad4(act_prev, h);
#pragma unroll
            for (int v = 0; v < 4; ++v) p[v * psh] = col < out_prev ? dg[j][v] * dh[v] : 0.f;
        }
    }
}

// Layer table + staging table of a network whose weight images all live in one CU's LDS.  Every width is padded to
// 16 * 2^j (compile-time contraction lengths); weight image [pout][pin + 4] (conflict-free 128-bit fragment reads), then the
// bias [pout].  tab: per 16-byte unit of the LDS image {source element offset into params or -1, LDS float offset |
// valid elements << 20 | 16-byte load legal << 24}; tab_begin[l] = first entry of layer l.  Returns false when a width
// does not qualify.  fl: floats of LDS the images take; per_wg: floats of one workgroup's gradient partials (dense).
inline bool snet_layout(const dcv_mlp* m, SnetLayer* ly, std::vector<int2>& tab, int* tab_begin, int& fl, int64_t& per_wg,
                        std::vector<int>* img_idx = nullptr) {
    if (img_idx) img_idx->assign((size_t)m->n_params, -1);
    fl = 0;
    per_wg = 0;
    int u4 = 0;
    for (int l = 0; l < m->L; ++l) {
        const LayerPlan& p = m->layers[l];
        SnetLayer& y = ly[l];
        y.in = p.in; y.out = p.out; y.act = p.act;
        auto pad = [](int w) { int k = 1; while (16 * k < w) k *= 2; return 16 * k; };
        y.pin = pad(p.in);
        y.pout = pad(p.out);
        if (y.pin > 256 || y.pout > 256) return false;
        y.nk_in = y.pin / 16;
        y.nk_out = y.pout / 16;
        y.u4_begin = u4;
        u4 += y.pout * (y.pin / 4);
        y.c4_shift = 0;
        while ((1 << y.c4_shift) < y.pin / 4) ++y.c4_shift;
        y.w_off = p.w_off; y.b_off = p.b_off;
        y.pws = y.pin + 4;
        y.lw = fl; fl += y.pout * y.pws;
        y.lb = fl; fl += y.pout;
        y.pw_off = y.pb_off = 0;
        y.pw_stride = (p.out * p.in + 3) / 4 * 4;
        y.pb_stride = (p.out + 3) / 4 * 4;
        per_wg += (int64_t)((p.out * p.in + 3) / 4 * 4) + (p.out + 3) / 4 * 4;
        if (tab_begin) tab_begin[l] = (int)tab.size();
        if (img_idx) {   // image float offset of every parameter of this layer
            for (int o = 0; o < p.out; ++o) {
                for (int i = 0; i < p.in; ++i) (*img_idx)[(size_t)(p.w_off + (int64_t)o * p.in + i)] = y.lw + o * y.pws + i;
                (*img_idx)[(size_t)(p.b_off + o)] = y.lb + o;
            }
        }
        const bool vec = (p.in % 4 == 0) && (p.w_off % 4 == 0);
        for (int o = 0; o < y.pout; ++o)
            for (int c = 0; c < y.pin / 4; ++c) {
                const int nv = o < p.out ? (p.in - 4 * c >= 4 ? 4 : (p.in - 4 * c > 0 ? p.in - 4 * c : 0)) : 0;
                tab.push_back(make_int2(nv > 0 ? (int)(p.w_off + (int64_t)o * p.in + 4 * c) : -1,
                                        (y.lw + o * y.pws + 4 * c) | (nv << 20) | ((vec && nv == 4 ? 1 : 0) << 24)));
            }
        for (int c = 0; c < y.pout / 4; ++c) {
            const int nv = p.out - 4 * c >= 4 ? 4 : (p.out - 4 * c > 0 ? p.out - 4 * c : 0);
            tab.push_back(make_int2(nv > 0 ? (int)(p.b_off + 4 * c) : -1, (y.lb + 4 * c) | (nv << 20) | ((nv == 4 && p.b_off % 4 == 0 ? 1 : 0) << 24)));
        }
    }
    return fl < (1 << 20) && m->n_params < (1ll << 31);
}

// Stages floats [f0, f1) of the global weight image (same layout as the LDS image; f0, f1 multiples of 256 floats are not
// required) into LDS with global_load_lds: no table, no VGPR, every copy of the workgroup in flight at once -- ONE round trip
// where the table-driven staging took two per pass of 12 units.  Completion: the caller's s_waitcnt vmcnt(0) + barrier.
template <int NT>
__device__ __forceinline__ void snet_stage_image(const float* __restrict__ img, float* sl, int f0, int f1, int t) {
    const int u0 = f0 >> 2, u1 = (f1 + 3) >> 2;
    for (int ub = u0 + (t & ~63); ub < u1; ub += NT) {   // a wave-instruction covers 64 consecutive 16-byte units
        const int u = ub + (t & 63);
        const unsigned ldsw = lds_addr_uniform(sl + 4 * ub);
        if (u < u1) glds16(img + 4 * u, ldsw);
    }
}

// ---- host side of the fused small-network plans

// Activation map of a TR-row tile: H_0 .. H_L from LDS float f on, row stride = padded width + 4 (H_0 = the input tile);
// returns the first float behind H_L
inline int snet_act_map(const SnetLayer* ly, int L, int TR, int f, int* lh, int* ps) {
    for (int l = 0; l <= L; ++l) {
        const int P = l == 0 ? ly[0].pin : ly[l - 1].pout;
        ps[l] = P + 4;
        lh[l] = f;
        f += TR * (P + 4);
    }
    return f;
}

// Where the nwg workgroups of a launch leave their gradient partials in `part` (16-byte aligned items: vector stores in the
// kernels, vector loads in the reduction), and the reduction's descriptors of them
inline void snet_partials_layout(SnetLayer* ly, int L, int64_t nwg, float* part, ReduceArgsView* ra) {
    int64_t off = 0;
    for (int l = 0; l < L; ++l) {
        SnetLayer& y = ly[l];
        y.pw_off = off; off += nwg * (int64_t)y.pw_stride;
        y.pb_off = off; off += nwg * (int64_t)y.pb_stride;
        if (ra) {
            ra->slab[l] = part + y.pw_off;
            ra->bpart[l] = part + y.pb_off;
            ra->splits[l] = (int)nwg;
            ra->bblocks[l] = (int)nwg;
            ra->wstride[l] = y.pw_stride;
            ra->bstride[l] = y.pb_stride;
        }
    }
}

// A device buffer of at least `need` elements (contents are not kept when it grows)
template <class T>
inline bool snet_grow(T** p, int64_t* have, int64_t need) {
    if (*have >= need) return true;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *have = 0;
    if (hipMalloc(reinterpret_cast<void**>(p), (size_t)need * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    *have = need;
    return true;
}

// Device copy of the staging table; on failure the caller releases *dev with the rest of its plan
inline bool snet_upload_table(const std::vector<int2>& tab, int2** dev) {
    if (hipMalloc(reinterpret_cast<void**>(dev), tab.size() * sizeof(int2)) == hipSuccess &&
        hipMemcpy(*dev, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice) == hipSuccess)
        return true;
    (void)hipGetLastError();
    return false;
}

// "Build the plan on first use": true when `plan` is there or `build` has just made it; one attempt per engine
template <class Build>
inline bool snet_plan_ready(const void* plan, bool& tried, Build&& build) {
    if (plan != nullptr) return true;
    const bool built = !tried && build();
    tried = true;
    return built;
}

// Launch of a fused kernel with up to lds_max bytes of dynamic LDS.  attr_state, one per kernel instantiation: 0 unknown,
// 1 the attribute is set, -1 refused by the runtime (the fused form is then off: returns 1)
template <class K, class Args>
inline int snet_launch(K kern, int& attr_state, size_t lds_max, size_t lds_bytes, const Args& a, int64_t nwg, hipStream_t s) {
    if (attr_state == 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
        if (e != hipSuccess) (void)hipGetLastError();
        attr_state = e == hipSuccess ? 1 : -1;
    }
    if (attr_state < 0) return 1;
    if (g_launch_ev.start != nullptr) {   // a profiled launch: events stamped with the kernel's own begin / end (common.h)
        const LaunchEvents ev = g_launch_ev;
        g_launch_ev = LaunchEvents{};
        g_launch_taken = ev.start;
        hipExtLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(kSnetThreads), (uint32_t)lds_bytes, s, ev.start, ev.stop, 0u, a);
    } else {
        hipLaunchKernelGGL(kern, dim3((unsigned)nwg), dim3(kSnetThreads), lds_bytes, s, a);
    }
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

inline bool snet_disabled() {
    static const bool off = env_is("DCV_NO_SNET", '1');
    return off;
}

}  // namespace dcv

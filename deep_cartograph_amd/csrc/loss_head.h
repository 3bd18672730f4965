// The loss head's arithmetic, one definition each, composed by every launch form of the head: the kernels of the
// layer-by-layer engine (mlp_heads.hip) and the tails of the fused small-network kernels (snet.hip, snet_dt.hip).
// A sum's order is part of the result: every form of a step must leave the bits of every other.
#pragma once
#include "common.h"
#include "handoff.h"
#include <math.h>

namespace dcv {

// ------------------------------------------------------------------ partial sums in a fixed order
// One wave adds n partials: lane l takes load(l), load(l + 64), ... in that order, then the shuffle-down tree; the sum is
// in lane 0.  `load` is a plain load, or handoff_load where the partials come from other workgroups of the same launch.
template <class Load>
__device__ __forceinline__ double wave_sum_in_order(Load load, int n, int lane) {
    double s = 0.0;
    for (int b = lane; b < n; b += 64) s += load(b);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;
}
// The last arriver of a ticketed reduction (handoff.h) adds part[nblocks][W]: the other blocks' partials come from memory
// (1-2 us each), so G thread groups take the blocks b = g, g + G, ... with eight loads in flight, added in block order, then
// thread t < W adds the G group sums in group order (fixed order: deterministic, the same sums whichever block is last).
// Whole workgroup, t = threadIdx.x, G * W <= the block size; s_grp: G * W doubles of LDS.  Returns the sum of column t < W.
__device__ __forceinline__ double block_sum_partials_in_order(const double* __restrict__ part, unsigned nblocks, int W, int G, int t,
                                                              double* __restrict__ s_grp) {
    const int g = t / W, o = t - g * W;
    if (g < G) {
        double s = 0.0;
        for (unsigned b0 = g; b0 < nblocks; b0 += 8 * G) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned b = b0 + (unsigned)u * G;
                v[u] = handoff_load(part + (int64_t)(b < nblocks ? b : b0) * W + o);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (b0 + (unsigned)u * G < nblocks) s += v[u];
        }
        s_grp[g * W + o] = s;
    }
    __syncthreads();
    double s = 0.0;
    if (t < W) {
#pragma unroll
        for (int q = 0; q < G; ++q) s += s_grp[q * W + t];
    }
    return s;
}

// ------------------------------------------------------------------ Deep-TICA batch statistics
// Entry o of [sum f_t | sum f_lag | sum f_t f_t^T | sum f_t f_lag^T] (2d + 2d^2 values) over nr pairs, float64, in pair
// order; ft(r, i) / fl(r, i): output i of pair r's f_t / f_lag row as a double.
template <class FT, class FL>
__device__ __forceinline__ double tica_stat_entry(int o, int d, int nr, FT ft, FL fl) {
    double s = 0.0;
    if (o < d) {
        for (int r = 0; r < nr; ++r) s += ft(r, o);
    } else if (o < 2 * d) {
        for (int r = 0; r < nr; ++r) s += fl(r, o - d);
    } else if (o < 2 * d + d * d) {
        const int q = o - 2 * d, i = q / d, j = q - i * d;
        for (int r = 0; r < nr; ++r) s += ft(r, i) * ft(r, j);
    } else {
        const int q = o - 2 * d - d * d, i = q / d, j = q - i * d;
        for (int r = 0; r < nr; ++r) s += ft(r, i) * fl(r, j);
    }
    return s;
}

// ------------------------------------------------------------------ autoencoder / VAE loss record
// rec = [recon (+ beta * kl / Bg) | weight Bg | VAE: recon | kl / Bg], recon = sse / (Bg * F), from the sums over the batch
__device__ __forceinline__ void ae_loss_record(double* __restrict__ rec, double sse, double kl, double Bg, int F, double beta, bool vae) {
    const double recon = sse / (Bg * (double)F);
    rec[0] = vae ? recon + beta * (kl / Bg) : recon;
    rec[1] = Bg;
    if (vae) {
        rec[2] = recon;
        rec[3] = kl / Bg;
    }
}

// ------------------------------------------------------------------ loss records of a batched pass
// A step appends one record at slot = the counter and moves the counter by one.  A batched evaluation (tica_stats_rows_group_kernel,
// snet_dt_fwd_kernel / snet_ae_kernel with nb > 1) appends in batch order: every member reads the counter, member j writes
// record (counter + j) through a log base moved by j records with the capacity left behind it.  The counter moves ONCE, by the
// group size: by the member that finishes last (log_advance_by_ticket) or by log_advance_kernel behind the launch.
struct MemberLog {
    double* log;   // this member's record lies at log + counter * log_width and exists when counter < cap
    int cap;
};
__device__ __forceinline__ MemberLog log_member(double* log, int log_width, int log_cap, int j) {
    return MemberLog{log + (int64_t)j * log_width, log_cap - j};
}
// the second ticket (zero between launches), taken behind the caller's read of the counter (slot0): the last of the
// `members` to take it moves the counter
__device__ __forceinline__ void log_advance_by_ticket(unsigned* ticket, int members, int* log_count, int slot0) {
    const unsigned prev = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == (unsigned)members - 1u) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *log_count = slot0 + members;
    }
}

// ------------------------------------------------------------------ Deep-TICA gradient row
// Gradient of the loss w.r.t. the network outputs from the head's matrices gradp = [mu d | Gu d*d | Gv d*d | c d]:
//   dL/df_t = c + Gu u + Gv v,   dL/df_lag = Gv u      (u = f_t - mu, v = f_lag - mu).
// Evaluated in float64 from the float64 batch statistics, rounded once: the loss does not change when a constant is
// added to the outputs, so the exact gradient rows sum to zero over the batch, and every parameter whose gradient is a
// multiple of that sum (the last bias; the bias of any hidden unit that stays on one side of its ReLU kink over the
// batch) has an exactly zero gradient.  Adam divides by |g| + 1e-8: a common-mode residue of 1e-5 -- what mu and the
// matrices rounded to float32 leave -- moves those parameters by a full +-lr per step, where autograd's
// (g - mean g) leaves 1e-10.  In float64 the rows sum to zero up to their own final rounding, as there.
struct TicaGradMats {
    const double *mu, *Gu, *Gv, *c;
};
__device__ __forceinline__ TicaGradMats tica_grad_mats(const double* gradp, int d) {
    return TicaGradMats{gradp, gradp + d, gradp + d + d * d, gradp + d + 2 * d * d};
}
// Component i of the two rows, one fma chain each in a fixed order: c, then per k the Gu u fma followed by the Gv v fma.
// f_own / f_lag / f_src: the d outputs of the row itself, of its pair's lagged row, of the row it is the lagged row of.
// KMAX > 0: k = 0 .. KMAX - 1 (the arrays' length) guarded by k < D, unrolled by recursion and not by `#pragma unroll`: the
// rows arrive as pointers to register arrays, and only indices that are constants when the call is inlined keep such an
// array out of scratch (an unrolled loop left 16 D + 16 bytes per lane in head_backward_kernel).  KMAX = 0: a run-time loop.
template <int KMAX, int K = 0, class Step>
__device__ __forceinline__ void tica_grad_k_loop(int D, Step step) {
    if constexpr (KMAX > 0) {
        if constexpr (K < KMAX) {
            if (K < D) step(K);
            tica_grad_k_loop<KMAX, K + 1>(D, step);
        }
    } else {
        for (int k = 0; k < D; ++k) step(k);
    }
}
template <int KMAX>
__device__ __forceinline__ double tica_grad_t(int i, int D, const double* mu, const double* Gu, const double* Gv, const double* c,
                                              const float* f_own, const float* f_lag) {
    double g = c[i];
    tica_grad_k_loop<KMAX>(D, [&](int k) {
        g = fma(Gu[i * D + k], (double)f_own[k] - mu[k], g);
        g = fma(Gv[i * D + k], (double)f_lag[k] - mu[k], g);
    });
    return g;
}
template <int KMAX>
__device__ __forceinline__ double tica_grad_l(int i, int D, const double* mu, const double* Gv, const float* f_src) {
    double g = 0.0;
    tica_grad_k_loop<KMAX>(D, [&](int k) { g = fma(Gv[i * D + k], (double)f_src[k] - mu[k], g); });
    return g;
}
// v[i] without a dynamically indexed register array (which would live in scratch); the same recursion
template <int N, int K = 1>
__device__ __forceinline__ float pick_from(int i, const float* v, float x) {
    if constexpr (K < N) return pick_from<N, K + 1>(i, v, i == K ? v[K] : x);
    else return x;
}
template <int N>
__device__ __forceinline__ float pick(int i, const float (&v)[N]) { return pick_from<N>(i, v, v[0]); }

// ------------------------------------------------------------------ the d x d Deep-TICA head on one wave
// The head (C0, Ctau, loss = -tr((A Ctau)^2), the gradient matrices: tica_grad_body in mlp_heads.hip is the single-thread
// form for any d) spread over the lanes of one wave (D <= 4: lane l < D*D owns matrix element (l / D, l % D)): the
// single-thread form is a chain of ~2000 dependent float64 instructions (8 us); here every matrix product is one step
// of D multiply-adds per lane and only the Cholesky factorisation (D columns) and the two triangular solves (one
// column of the inverse per lane) stay sequential.  Matrices live in LDS; the wave is its own barrier.
template <int D>
struct TicaWaveLds {
    double mu[D], ml[D], invL[D];
    double C0[D * D], Ct[D * D], L[D * D], A[D * D], K[D * D], T[D * D];
};
__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int D>
__device__ __forceinline__ void tica_grad_wave(TicaWaveLds<D>& w, const double* __restrict__ stats, double Bg, double reg,
                                               double* __restrict__ gradp, double* __restrict__ log, int* __restrict__ log_count,
                                               int log_cap, int log_width, int lane) {
    const int i = lane / D, j = lane % D;
    const bool el = lane < D * D;
    const double invB = 1.0 / Bg;
    const double* Stt = stats + 2 * D;
    const double* Stl = stats + 2 * D + D * D;
    if (lane < D) {
        w.mu[lane] = stats[lane] * invB;
        w.ml[lane] = stats[D + lane] * invB;
    }
    wave_sync_lds();
    if (el) {
        w.C0[lane] = 0.5 * (Stt[i * D + j] + Stt[j * D + i]) * invB - w.mu[i] * w.mu[j];
        const double cij = Stl[i * D + j] * invB - w.mu[i] * w.ml[j];
        const double cji = Stl[j * D + i] * invB - w.mu[j] * w.ml[i];
        w.Ct[lane] = 0.5 * (cij + cji);
        w.L[lane] = 0.0;
    }
    wave_sync_lds();
    // Cholesky of C0 + reg I, column by column
    bool ok = true;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        if (lane == 0) {
            double s = w.C0[k * D + k] + reg;
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m < k) s -= w.L[k * D + m] * w.L[k * D + m];
            const double lkk = sqrt(s);
            w.L[k * D + k] = lkk;
            w.invL[k] = s > 0.0 ? 1.0 / lkk : NAN;
        }
        wave_sync_lds();
        if (lane < D && lane > k) {   // L[lane][k]
            double s = w.C0[lane * D + k];
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m < k) s -= w.L[lane * D + m] * w.L[k * D + m];
            w.L[lane * D + k] = s * w.invL[k];
        }
        wave_sync_lds();
    }
#pragma unroll
    for (int k = 0; k < D; ++k) ok = ok && !(w.invL[k] != w.invL[k]);
    // A = (L L^T)^-1: lane c < D solves L y = e_c, L^T a = y (column c of A)
    if (lane < D) {
        const int c = lane;
        double y[D], a[D];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            double s = (r == c) ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m < r) s -= w.L[r * D + m] * y[m];
            y[r] = s * w.invL[r];
        }
#pragma unroll
        for (int rr = 0; rr < D; ++rr) {
            const int r = D - 1 - rr;
            double s = y[r];
#pragma unroll
            for (int m = 0; m < D; ++m)
                if (m > r) s -= w.L[m * D + r] * a[m];
            a[r] = s * w.invL[r];
        }
#pragma unroll
        for (int r = 0; r < D; ++r) w.A[r * D + c] = a[r];
    }
    wave_sync_lds();
    if (el) {   // K = A Ct
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) s += w.A[i * D + m] * w.Ct[m * D + j];
        w.K[lane] = s;
    }
    wave_sync_lds();
    double Tij = 0.0;
    if (el) {   // T = K A (= A Ct A)
#pragma unroll
        for (int m = 0; m < D; ++m) Tij += w.K[i * D + m] * w.A[m * D + j];
        w.T[lane] = Tij;
    }
    wave_sync_lds();
    if (gradp && el) {
        double g0 = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) g0 += w.K[i * D + m] * w.T[m * D + j];
        const double Gt = -(w.T[i * D + j] + w.T[j * D + i]);
        gradp[D + lane] = 4.0 * g0 * invB;               // (2/B) G0, G0 = 2 K T
        gradp[D + D * D + lane] = Gt * invB;             // (1/B) Gtau
    }
    if (gradp && lane < D) {
        gradp[lane] = w.mu[lane];
        double cs = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) cs += -(w.T[lane * D + m] + w.T[m * D + lane]) * (w.ml[m] - w.mu[m]);
        gradp[D + 2 * D * D + lane] = -cs * invB;
    }
    if (log_count == nullptr) return;   // no record asked for (the workgroups of a fused backward other than the first)
    const int slot = *log_count;
    if (slot < log_cap) {
        double* rec = log + (int64_t)slot * log_width;
        if (lane == 0) {
            double loss = 0.0;   // -tr(K K), summed in the order of the single-thread form
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) loss -= w.K[a * D + b] * w.K[b * D + a];
            rec[0] = ok ? loss : NAN;
            rec[1] = Bg;
        }
        if (el) {
            rec[2 + lane] = w.C0[lane];
            rec[2 + D * D + lane] = w.Ct[lane];
        }
        if (lane < D) rec[2 + 2 * D * D + lane] = w.mu[lane];
    }
    wave_sync_lds();
    if (lane == 0) *log_count = slot + 1;
}

// what the last arriver of a ticketed statistics reduction goes on to do (one-GPU steps: the loss head in the same launch)
struct FusedHead {
    int on;            // wave 0 of the last block runs tica_grad_wave on the summed statistics
    double Bg, reg;
    double* gradp;     // null: evaluation only
    double* log;
    int* log_count;
    int log_cap, log_width;
};

}  // namespace dcv

// Frame interpolation of a trajectory (traj_augmentation): a shape-preserving cubic -- PCHIP or modified Akima
// ("makima") -- through every coordinate column along the frame axis, evaluated at new times.  n_knots x atoms x 3
// float32 in, n_out x selected atoms x 3 float32 out, float64 arithmetic in between (the formulas: include/dcv.h).
//
// Columns are independent and an output needs the 4 (PCHIP) or 6 (makima) knots around its time, so this is a
// streaming stencil along time and nothing is staged in LDS: there is no limit on the number of atoms.  A WAVE owns 64
// adjacent coordinate columns (consecutive lanes on consecutive addresses of the output, dense rows or DCD planes
// alike; on those of the noise when there is noise) and a run of consecutive output frames; a workgroup is four such
// waves with nothing shared between them.  The times of a run are the same for every lane (scalar loads, four at a
// time and one group ahead), so the interval index K = floor(t) moves for the whole wave at once: no divergence.  A
// lane keeps the six knots y[K-2 .. K+3] of its column in registers as float64, plus the next one (y[K+4], loaded when
// the window last moved, i.e. one interval ahead of need), the four coefficients of the current piece and the
// derivative at its right knot, which is the left one of the next piece; when K advances it shifts the window, takes
// the knot that is already there and issues the load of the following one.  The knots are read with one 4-byte load per lane (256 contiguous bytes per
// wave and row where the selection is contiguous): rows start at any alignment and a selection gathers, and each lane
// reads a knot once per run; the stores are the traffic that matters and go out as 256 contiguous bytes per wave.
//
// makima needs G, the largest f1 + f2 of ALL selected columns (scipy's threshold is global): interp_gmax_kernel walks
// the knots the same way, reduces over the lanes with shuffles and writes one partial per wave with a plain store; a
// one-workgroup launch reduces the partials.  A maximum does not depend on the order: bit-identical from run to run.
// No atomics, no hand-offs between workgroups.
#include <cmath>
#include <vector>

#include "coords.h"

namespace dcv {

constexpr int kInterpThreads = 256;
constexpr int kInterpWaves = kInterpThreads / kWave;   // independent waves of a workgroup
constexpr int kInterpMinRun = 64;                      // output frames (or knots) of a run: the 6 knots of warm-up stay below 10 % of its traffic
constexpr int64_t kInterpTargetWaves = 8192;           // 256 CUs x 4 SIMDs x 8 waves
constexpr int kInterpGroup = 4;                        // times per group of scalar loads

struct InterpArgs {
    const float* xyz;
    int64_t n_knots;
    CoordStrides in;
    const int32_t* sel;        // n_sel atoms or NULL (atom s is atom s)
    int64_t n_sel, n_cols;     // n_cols = 3 n_sel
    int32_t comp_fast;         // column q is (atom q / 3, component q % 3); otherwise (atom q % n_sel, component q / n_sel)
    int32_t extrapolate;
    const double* t;           // n_out times
    int64_t n_out;
    const double* noise;       // n_out x n_sel x 3 or NULL
    float* out;
    CoordStrides outs;         // of the output
    int64_t runs, run_len, n_tasks;   // a task = (column block, run); runs of run_len outputs (knots in the G pass)
    double* partials;          // G pass: one maximum per task
    const double* G;           // evaluation: the reduced maximum (makima)
};

struct InterpColumn {
    const float* in;
    float* out;
    const double* noise;
};

__device__ __forceinline__ InterpColumn interp_column(const InterpArgs& a, int64_t q) {
    int64_t s, c;
    if (a.comp_fast) { s = q / 3; c = q - 3 * s; }
    else { c = q / a.n_sel; s = q - c * a.n_sel; }
    const int64_t atom = a.sel ? (int64_t)a.sel[s] : s;
    InterpColumn col;
    col.in = a.xyz + atom * a.in.a + c * a.in.c;
    col.out = a.out ? a.out + s * a.outs.a + c * a.outs.c : nullptr;
    col.noise = a.noise ? a.noise + 3 * s + c : nullptr;
    return col;
}

// knot k of a column, 0 outside the trajectory (such a value is never used: the end rules replace what it feeds)
__device__ __forceinline__ float interp_knot(const InterpArgs& a, const float* col, int64_t k) {
    return k >= 0 && k < a.n_knots ? col[k * a.in.f] : 0.0f;
}

__device__ __forceinline__ void interp_window(const InterpArgs& a, const float* col, int64_t K, double (&w)[6], float& nxt) {
    float v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] = interp_knot(a, col, K - 2 + i);
    nxt = interp_knot(a, col, K + 4);
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = (double)v[i];
}

__device__ __forceinline__ void interp_advance(const InterpArgs& a, const float* col, int64_t& K, double (&w)[6], float& nxt) {
#pragma unroll
    for (int i = 0; i < 5; ++i) w[i] = w[i + 1];
    w[5] = (double)nxt;
    ++K;
    nxt = interp_knot(a, col, K + 4);
}

// numpy.sign: NaN for NaN, so that a != of two signs is true whenever one of them is NaN
__device__ __forceinline__ double interp_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

__device__ __forceinline__ double pchip_interior(double ma, double mb) {
#pragma clang fp contract(off)
    if (interp_sign(ma) != interp_sign(mb) || ma == 0.0 || mb == 0.0) return 0.0;
    return 1.0 / ((3.0 / ma + 3.0 / mb) / 6.0);
}

__device__ __forceinline__ double pchip_end(double m0, double m1) {
#pragma clang fp contract(off)
    const double e = (3.0 * m0 - m1) / 2.0;
    if (interp_sign(e) != interp_sign(m0)) return 0.0;
    if (interp_sign(m0) != interp_sign(m1) && fabs(e) > 3.0 * fabs(m0)) return 3.0 * m0;
    return e;
}

// The five slopes m_{K-2} .. m_{K+2} of the window, with makima's linear continuation past both ends.  K is the same in
// every lane of a wave.
__device__ __forceinline__ void makima_slopes(const double (&w)[6], int64_t K, int64_t n, double (&sl)[5]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 5; ++i) sl[i] = w[i + 1] - w[i];
    if (K == 0) { sl[1] = 2.0 * sl[2] - sl[3]; sl[0] = 2.0 * sl[1] - sl[2]; }
    else if (K == 1) sl[0] = 2.0 * sl[1] - sl[2];
    if (K == n - 2) { sl[3] = 2.0 * sl[2] - sl[1]; sl[4] = 2.0 * sl[3] - sl[2]; }
    else if (K == n - 3) sl[4] = 2.0 * sl[3] - sl[2];
}

__device__ __forceinline__ void makima_weights(double m0, double m1, double m2, double m3, double& f1, double& f2) {
#pragma clang fp contract(off)
    f1 = fabs(m3 - m2) + 0.5 * fabs(m3 + m2);
    f2 = fabs(m1 - m0) + 0.5 * fabs(m1 + m0);
}

__device__ __forceinline__ double makima_derivative(double m0, double m1, double m2, double m3, double thr) {
#pragma clang fp contract(off)
    double f1, f2;
    makima_weights(m0, m1, m2, m3, f1, f2);
    const double f12 = f1 + f2;
    return f12 > thr ? (f1 * m1 + f2 * m2) / f12 : 0.5 * (m3 + m0);
}

// Coefficients of the piece on [K, K + 1]: p = c[0] + c[1] s + c[2] s^2 + c[3] s^3; y1 = y[K + 1].  d1 carries the
// derivative at the right knot from piece to piece: with `carry` (the window moved by exactly one knot) it arrives as
// d_K -- the same operations on the same slopes, the padded ones included -- and only d_{K+1} is computed.
template <int KIND>
__device__ __forceinline__ void interp_piece(const double (&w)[6], int64_t K, int64_t n, double thr, bool carry, double& d1, double (&c)[4],
                                             double& y1) {
#pragma clang fp contract(off)
    double d0 = d1;
    const double m = w[3] - w[2];
    if (KIND == DCV_INTERP_PCHIP) {
        const double ml = w[2] - w[1], mr = w[4] - w[3];
        if (n == 2) { d0 = m; d1 = m; }
        else {
            if (!carry) d0 = K == 0 ? pchip_end(m, mr) : pchip_interior(ml, m);
            d1 = K == n - 2 ? pchip_end(m, ml) : pchip_interior(m, mr);
        }
    } else {
        double sl[5];
        makima_slopes(w, K, n, sl);
        if (!carry) d0 = makima_derivative(sl[0], sl[1], sl[2], sl[3], thr);
        d1 = makima_derivative(sl[1], sl[2], sl[3], sl[4], thr);
    }
    const double T = d0 + d1 - 2.0 * m;
    c[0] = w[2]; c[1] = d0; c[2] = (m - d0) - T; c[3] = T;
    y1 = w[3];
}

__device__ __forceinline__ int64_t interp_interval(double t, int64_t n) {
    const double f = floor(t), hi = (double)(n - 2);
    return (int64_t)(f < 0.0 ? 0.0 : (f > hi ? hi : f));
}

template <int KIND>
__global__ __launch_bounds__(kInterpThreads) void interp_kernel(const InterpArgs a) {
#pragma clang fp contract(off)   // the arithmetic of NumPy, operation by operation
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t task = (int64_t)blockIdx.x * kInterpWaves + wave;
    if (task >= a.n_tasks) return;
    const int64_t cb = task / a.runs, run = task - cb * a.runs;
    const int64_t q = cb * kWave + lane;
    if (q >= a.n_cols) return;   // no barrier and no shuffle below
    const InterpColumn col = interp_column(a, q);
    const int64_t n = a.n_knots;
    const int64_t j0 = run * a.run_len, j1 = j0 + a.run_len < a.n_out ? j0 + a.run_len : a.n_out;
    const double thr = KIND == DCV_INTERP_MAKIMA ? 1e-9 * a.G[0] : 0.0;
    const double last = (double)(n - 1);

    // the times come in groups of kInterpGroup scalar loads, the next group in flight under the current one (the array
    // is padded by two groups, so a group past the end of the run is readable and never used)
    double tn[kInterpGroup];
#pragma unroll
    for (int u = 0; u < kInterpGroup; ++u) tn[u] = a.t[j0 + u];
    int64_t K = interp_interval(tn[0], n);
    double w[6], c[4], y1, d1 = 0.0;
    float nxt;
    interp_window(a, col.in, K, w, nxt);
    interp_piece<KIND>(w, K, n, thr, false, d1, c, y1);
    for (int64_t jg = j0; jg < j1; jg += kInterpGroup) {
        double tc[kInterpGroup];
#pragma unroll
        for (int u = 0; u < kInterpGroup; ++u) { tc[u] = tn[u]; tn[u] = a.t[jg + kInterpGroup + u]; }
#pragma unroll
        for (int u = 0; u < kInterpGroup; ++u) {
            const int64_t j = jg + u;
            if (j >= j1) break;
            const double t = tc[u];
            const int64_t Kn = interp_interval(t, n);
            if (Kn != K) {   // the same in every lane
                const bool carry = Kn - K == 1;
                if (Kn - K >= 6) { K = Kn; interp_window(a, col.in, K, w, nxt); }
                else while (K < Kn) interp_advance(a, col.in, K, w, nxt);
                interp_piece<KIND>(w, K, n, thr, carry, d1, c, y1);
            }
            const double s = t - (double)K;
            // scipy's PPoly: the powers by repeated multiplication, the terms added from the constant up
            const double z2 = s * s, z3 = z2 * s;
            double p = c[0] + c[1] * s;
            p += c[2] * z2;
            p += c[3] * z3;
            if (s == 1.0 && p == p) p = y1;   // the last knot is the right end of its piece
            if (!a.extrapolate && (t < 0.0 || t > last)) p = __builtin_nan("");
            if (col.noise) p += col.noise[j * a.n_cols];
            col.out[j * a.outs.f] = (float)p;
        }
    }
}

// makima: the largest finite f1 + f2 over the knots of a run, over the 64 columns of the wave
__global__ __launch_bounds__(kInterpThreads) void interp_gmax_kernel(const InterpArgs a) {
#pragma clang fp contract(off)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t task = (int64_t)blockIdx.x * kInterpWaves + wave;
    if (task >= a.n_tasks) return;   // whole waves leave
    const int64_t cb = task / a.runs, run = task - cb * a.runs;
    const int64_t q = cb * kWave + lane;
    const int64_t n = a.n_knots;
    const int64_t K0 = run * a.run_len, K1 = K0 + a.run_len < n - 1 ? K0 + a.run_len : n - 1;   // intervals [K0, K1) of 0 .. n - 2
    double mx = -INFINITY;
    if (q < a.n_cols) {
        const InterpColumn col = interp_column(a, q);
        int64_t K = K0;
        double w[6];
        float nxt;
        interp_window(a, col.in, K, w, nxt);
        while (true) {
            double sl[5], f1, f2;
            makima_slopes(w, K, n, sl);
            makima_weights(sl[0], sl[1], sl[2], sl[3], f1, f2);
            double f12 = f1 + f2;
            if (isfinite(f12)) mx = fmax(mx, f12);
            if (K == n - 2) {   // the last knot has no interval of its own
                makima_weights(sl[1], sl[2], sl[3], sl[4], f1, f2);
                f12 = f1 + f2;
                if (isfinite(f12)) mx = fmax(mx, f12);
            }
            if (K + 1 >= K1) break;
            interp_advance(a, col.in, K, w, nxt);
        }
    }
    for (int m = kWave >> 1; m > 0; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m, kWave));
    if (lane == 0) a.partials[task] = mx;
}

__global__ __launch_bounds__(kInterpThreads) void interp_gmax_reduce_kernel(const double* partials, int64_t n, double* G) {
    __shared__ double sm[kInterpThreads];
    double mx = -INFINITY;
    for (int64_t i = threadIdx.x; i < n; i += kInterpThreads) mx = fmax(mx, partials[i]);
    sm[threadIdx.x] = mx;
    __syncthreads();
    for (int m = kInterpThreads >> 1; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + m]);
        __syncthreads();
    }
    if (threadIdx.x == 0) G[0] = sm[0];
}

// Host side: how the columns and the frames are dealt to waves, and the workspace.
struct InterpPlan {
    int64_t n_sel, n_cols, col_blocks;
    int64_t runs, run_len, n_tasks;      // evaluation
    int64_t kruns, krun_len, k_tasks;    // G pass over the n_knots - 1 intervals
    size_t t, sel, partials, G, total;   // byte offsets into the workspace
};

static void interp_deal(int64_t items, int64_t col_blocks, int64_t& runs, int64_t& run_len) {
    const int64_t want = cdiv(kInterpTargetWaves, col_blocks), most = cdiv(items, kInterpMinRun);
    runs = want < most ? want : most;
    if (runs < 1) runs = 1;
    run_len = cdiv(items, runs);
    if (run_len < 1) run_len = 1;
    runs = items > 0 ? cdiv(items, run_len) : 1;
}

static InterpPlan interp_plan(int64_t n_knots, int32_t n_atoms, int32_t n_sel, int64_t n_out) {
    InterpPlan p{};
    p.n_sel = n_sel > 0 ? n_sel : n_atoms;
    p.n_cols = 3 * p.n_sel;
    p.col_blocks = cdiv(p.n_cols, kWave);
    interp_deal(n_out, p.col_blocks, p.runs, p.run_len);
    p.n_tasks = p.col_blocks * p.runs;
    interp_deal(n_knots - 1, p.col_blocks, p.kruns, p.krun_len);
    p.k_tasks = p.col_blocks * p.kruns;
    size_t o = 0;
    p.t = o; o += align_up((size_t)(n_out + 2 * kInterpGroup) * sizeof(double), 256);   // padded: interp_kernel reads whole groups
    p.sel = o; o += align_up((size_t)p.n_sel * sizeof(int32_t), 256);
    p.partials = o; o += align_up((size_t)p.k_tasks * sizeof(double), 256);
    p.G = o; o += 256;
    p.total = o;
    return p;
}

}  // namespace dcv

using namespace dcv;

extern "C" size_t dcv_interpolate_workspace(int64_t n_knots, int32_t n_atoms, int32_t n_sel, int64_t n_out) {
    if (n_knots < 2 || n_atoms <= 0 || n_out < 0) return 0;
    return interp_plan(n_knots, n_atoms, n_sel, n_out).total;
}

extern "C" int dcv_interpolate(const float* xyz_d, int64_t n_knots, int64_t frame_stride, int64_t atom_stride, int64_t comp_stride,
                               int32_t n_atoms, const int32_t* sel_h, int32_t n_sel, int32_t kind, int32_t extrapolate,
                               const double* t_h, int64_t n_out, const double* noise_d, float* out_d, int64_t out_frame_stride,
                               int64_t out_atom_stride, int64_t out_comp_stride, void* ws_d, size_t ws_bytes, void* stream) {
    // ---- validate everything before anything is launched
    DCV_REQUIRE(kind == DCV_INTERP_PCHIP || kind == DCV_INTERP_MAKIMA, "dcv_interpolate: unknown kind %d", kind);
    DCV_REQUIRE(xyz_d && n_atoms > 0 && n_out >= 0 && (n_out == 0 || (t_h && out_d)),
                "dcv_interpolate: bad arguments (n_atoms=%d n_out=%lld)", n_atoms, (long long)n_out);
    DCV_REQUIRE(n_knots >= (kind == DCV_INTERP_MAKIMA ? 3 : 2), "dcv_interpolate: %lld knots, %s needs at least %d", (long long)n_knots,
                kind == DCV_INTERP_MAKIMA ? "makima" : "pchip", kind == DCV_INTERP_MAKIMA ? 3 : 2);
    DCV_REQUIRE(!sel_h || n_sel >= 1, "dcv_interpolate: a selection of %d atoms", n_sel);
    DCV_REQUIRE_COORD_STRIDES("dcv_interpolate", frame_stride, atom_stride, comp_stride);
    const CoordStrides in{frame_stride, atom_stride, comp_stride}, outs{out_frame_stride, out_atom_stride, out_comp_stride};
    DCV_REQUIRE_STRIDES_GE1("dcv_interpolate", "output strides", outs);
    if (sel_h)
        for (int32_t i = 0; i < n_sel; ++i)
            DCV_REQUIRE(sel_h[i] >= 0 && sel_h[i] < n_atoms, "dcv_interpolate: selected atom %d is %d, outside [0, %d)", i, sel_h[i], n_atoms);
    for (int64_t j = 0; j < n_out; ++j) {
        DCV_REQUIRE(std::isfinite(t_h[j]), "dcv_interpolate: time %lld is %g: the times must be finite", (long long)j, t_h[j]);
        DCV_REQUIRE(j == 0 || t_h[j] >= t_h[j - 1], "dcv_interpolate: time %lld (%g) is below time %lld (%g): the times must not decrease",
                    (long long)j, t_h[j], (long long)(j - 1), t_h[j - 1]);
    }
    const InterpPlan p = interp_plan(n_knots, n_atoms, sel_h ? n_sel : 0, n_out);
    DCV_REQUIRE(cdiv(p.n_tasks, kInterpWaves) <= 0x7fffffffLL && cdiv(p.k_tasks, kInterpWaves) <= 0x7fffffffLL,
                "dcv_interpolate: %lld columns x %lld frames need more than 2^31 - 1 workgroups", (long long)p.n_cols, (long long)n_out);
    DCV_REQUIRE_WORKSPACE("dcv_interpolate", ws_d, ws_bytes, p.total);
    if (n_out == 0) return DCV_OK;
    int64_t in_last, out_last;
    DCV_REQUIRE_COORDS_FIT("dcv_interpolate", coord_extent(n_knots, n_atoms, in, in_last), n_knots, n_atoms);
    DCV_REQUIRE_COORDS_FIT("dcv_interpolate", coord_extent(n_out, p.n_sel, outs, out_last), n_out, (int)p.n_sel);

    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(ws_d);
    // pageable sources: the runtime has taken its copy of both arrays when these calls return
    DCV_CHECK_HIP(hipMemcpyAsync(ws + p.t, t_h, (size_t)n_out * sizeof(double), hipMemcpyHostToDevice, s));
    if (sel_h) DCV_CHECK_HIP(hipMemcpyAsync(ws + p.sel, sel_h, (size_t)n_sel * sizeof(int32_t), hipMemcpyHostToDevice, s));

    InterpArgs a{};
    a.xyz = xyz_d;
    a.n_knots = n_knots; a.in = in;
    a.sel = sel_h ? reinterpret_cast<const int32_t*>(ws + p.sel) : nullptr;
    a.n_sel = p.n_sel; a.n_cols = p.n_cols;
    // lanes along consecutive addresses of the output; with noise along those of the noise, which is twice the bytes (a
    // wave then writes DCD planes as three pieces of 21 or 22 atoms: measured faster than reading every third double)
    a.comp_fast = coord_comp_fast(outs) || noise_d != nullptr;
    a.extrapolate = extrapolate;
    a.t = reinterpret_cast<const double*>(ws + p.t);
    a.n_out = n_out;
    a.noise = noise_d;
    a.out = out_d;
    a.outs = outs;
    a.partials = reinterpret_cast<double*>(ws + p.partials);
    a.G = reinterpret_cast<const double*>(ws + p.G);
    if (kind == DCV_INTERP_MAKIMA) {
        a.runs = p.kruns; a.run_len = p.krun_len; a.n_tasks = p.k_tasks;
        hipLaunchKernelGGL(interp_gmax_kernel, dim3((unsigned)cdiv(p.k_tasks, kInterpWaves)), dim3(kInterpThreads), 0, s, a);
        DCV_CHECK_LAUNCH();
        hipLaunchKernelGGL(interp_gmax_reduce_kernel, dim3(1), dim3(kInterpThreads), 0, s, a.partials, p.k_tasks, reinterpret_cast<double*>(ws + p.G));
        DCV_CHECK_LAUNCH();
    }
    a.runs = p.runs; a.run_len = p.run_len; a.n_tasks = p.n_tasks;
    const dim3 grid((unsigned)cdiv(p.n_tasks, kInterpWaves));
    if (kind == DCV_INTERP_MAKIMA) hipLaunchKernelGGL(interp_kernel<DCV_INTERP_MAKIMA>, grid, dim3(kInterpThreads), 0, s, a);
    else hipLaunchKernelGGL(interp_kernel<DCV_INTERP_PCHIP>, grid, dim3(kInterpThreads), 0, s, a);
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

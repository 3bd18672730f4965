// Shared helpers for libdcv.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/dcv.h"

namespace dcv {

void set_error(const char* fmt, ...);

#define DCV_CHECK_HIP(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) {                                                          \
            dcv::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return DCV_EHIP;                                                             \
        }                                                                                \
    } while (0)

#define DCV_REQUIRE(cond, ...)                                                           \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            dcv::set_error(__VA_ARGS__);                                                 \
            return DCV_EINVAL;                                                           \
        }                                                                                \
    } while (0)

// the workspace of `entry` (its name, a string literal) holds `need` bytes; callers put their own conditions around it
#define DCV_REQUIRE_WORKSPACE(entry, ws_d, ws_bytes, need)                                \
    do {                                                                                 \
        if (!(ws_d) || (ws_bytes) < (need)) {                                            \
            dcv::set_error(entry ": workspace too small (%zu bytes, need %zu)", (size_t)(ws_bytes), (size_t)(need)); \
            return DCV_ENOMEM;                                                           \
        }                                                                                \
    } while (0)

#define DCV_CHECK_LAUNCH() DCV_CHECK_HIP(hipGetLastError())

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
__host__ __device__ inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr int kWave = 64;  // gfx950 wavefront

// The rule for 16-byte accesses, decided on the host, in its one place.  aligned16: a vector read from its
// base; quad_ok: the rows of a matrix with row stride ld; quad_path: and its width F, so that no quad straddles a row's end.
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool quad_ok(const void* p, int64_t ld) { return ld % 4 == 0 && aligned16(p); }
inline bool quad_path(const void* p, int64_t F, int64_t ld) { return F % 4 == 0 && quad_ok(p, ld); }

// a workgroup's contiguous range [begin, end) of n rows or points: rows_per_block each, or an even share of the grid
struct Range {
    int64_t begin, end;
};
__device__ __forceinline__ Range block_rows(int64_t n, int64_t rows_per_block) {
    const int64_t begin = (int64_t)blockIdx.x * rows_per_block;
    return {begin, begin + rows_per_block < n ? begin + rows_per_block : n};
}
__device__ __forceinline__ Range block_range(int64_t n) { return block_rows(n, cdiv(n, gridDim.x)); }

// Kernel-exact timing of ONE launch (dcv_mlp_profile_*): the caller parks a pair of events here, the block engine's launcher
// hands them to hipExtLaunchKernel, which stamps them with the kernel's own begin / end (the interval rocprofv3 reports:
// events recorded around a launch also bracket the command processor's work between launches, 3-4 us at the contract batch),
// and clears the slot.  A slot nobody consumed (a launch that does not go through the block engine) is noticed by the
// caller, which then falls back to recording its events around the launch.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchEvents g_launch_ev;
extern thread_local hipEvent_t g_launch_taken;   // start event of the pair the launcher consumed last
// Number of CUs of the current device (cached).
int num_cus();
// Run-time switches (environment DCV_...).  Callers keep the answer in a `static const`: every switch is read once per
// process.  env_is: set and starting with `c` (an opt-in tests '1', an opt-out of a default '0'); env_not: its negation
// (on unless the value starts with `c`); env_int: atoll of the value, `unset` when the variable is not set.
bool env_is(const char* name, char c);
bool env_not(const char* name, char c);
int64_t env_int(const char* name, int64_t unset);
// arithmetic of the matrix products: false = FP32-input MFMA, true = FP32-accurate split products on the BF16
// matrix pipe (default; dcv_set_gemm_mode / environment DCV_GEMM_MODE=native|split)
bool gemm_split();
void set_gemm_split(bool on);

// Test hook (dcv_debug_gemm_log_*): host-side record of the product plans the block engine's launchers enqueued, so that a
// test can assert which tile family, loader and arithmetic flavour a shape reached instead of assuming it.  Fixed capacity;
// entries behind it are dropped.  Written on the host by the launch wrappers only: no kernel knows of it.
enum GemmLaunchForm { kFormSingle = 0, kFormGroup = 1, kFormPair = 2, kFormRide = 3 };
void gemm_log_push(int form, int mode, int tm, int tn, bool split, bool vec, bool gather, int64_t splits, int tail_split);

}  // namespace dcv

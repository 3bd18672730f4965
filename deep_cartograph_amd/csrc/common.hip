#include "common.h"
#include <string.h>
#include <stdlib.h>
#include <atomic>

namespace dcv {
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int num_cus() {
    static int cached = 0;
    if (cached) return cached;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    cached = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return cached;
}

bool env_is(const char* name, char c) {
    const char* e = getenv(name);
    return e && e[0] == c;
}
bool env_not(const char* name, char c) { return !env_is(name, c); }
int64_t env_int(const char* name, int64_t unset) {
    const char* e = getenv(name);
    return e ? (int64_t)atoll(e) : unset;
}

thread_local LaunchEvents g_launch_ev;
thread_local hipEvent_t g_launch_taken = nullptr;
static int g_gemm_split = -1;   // -1: not decided yet (environment, else the default)
bool gemm_split() {
    if (g_gemm_split < 0) {
        const char* e = getenv("DCV_GEMM_MODE");
        g_gemm_split = (e && strcmp(e, "native") == 0) ? 0 : 1;
    }
    return g_gemm_split == 1;
}
void set_gemm_split(bool on) { g_gemm_split = on ? 1 : 0; }

// ---- launch-plan log (common.h).  A full log costs a launch one relaxed load.
constexpr int kGemmLogCap = 256, kGemmLogFields = 9;
static int32_t g_gemm_log[kGemmLogCap][kGemmLogFields];
static std::atomic<int> g_gemm_log_n{0};
void gemm_log_push(int form, int mode, int tm, int tn, bool split, bool vec, bool gather, int64_t splits, int tail_split) {
    if (g_gemm_log_n.load(std::memory_order_relaxed) >= kGemmLogCap) return;
    const int i = g_gemm_log_n.fetch_add(1, std::memory_order_relaxed);
    if (i >= kGemmLogCap) {   // lost a race for the last slot
        g_gemm_log_n.store(kGemmLogCap, std::memory_order_relaxed);
        return;
    }
    int32_t* e = g_gemm_log[i];
    e[0] = form; e[1] = mode; e[2] = tm; e[3] = tn; e[4] = split; e[5] = vec; e[6] = gather;
    e[7] = (int32_t)splits; e[8] = tail_split;
}
}  // namespace dcv

extern "C" void dcv_debug_gemm_log_reset(void) { dcv::g_gemm_log_n.store(0); }
extern "C" int32_t dcv_debug_gemm_log_read(int32_t* out, int32_t cap) {
    const int n = dcv::g_gemm_log_n.load() < dcv::kGemmLogCap ? dcv::g_gemm_log_n.load() : dcv::kGemmLogCap;
    for (int i = 0; out != nullptr && i < n && i < cap; ++i) memcpy(out + (size_t)i * dcv::kGemmLogFields, dcv::g_gemm_log[i], sizeof(dcv::g_gemm_log[i]));
    return n;
}

extern "C" int dcv_set_gemm_mode(int mode) {
    DCV_REQUIRE(mode == DCV_GEMM_NATIVE_F32 || mode == DCV_GEMM_SPLIT_BF16X6, "dcv_set_gemm_mode: unknown mode %d", mode);
    dcv::set_gemm_split(mode == DCV_GEMM_SPLIT_BF16X6);
    return DCV_OK;
}
extern "C" int dcv_get_gemm_mode(void) { return dcv::gemm_split() ? DCV_GEMM_SPLIT_BF16X6 : DCV_GEMM_NATIVE_F32; }

extern "C" int dcv_abi_version(void) { return DCV_ABI_VERSION; }
extern "C" const char* dcv_last_error(void) { return dcv::g_err; }

extern "C" int dcv_device_info(int device, int* n_cu, int64_t* hbm_bytes, char* name, size_t name_len) {
    hipDeviceProp_t prop;
    DCV_CHECK_HIP(hipGetDeviceProperties(&prop, device));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (name && name_len) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    return DCV_OK;
}

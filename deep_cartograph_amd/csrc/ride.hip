// Grouped launch of the layer-0 weight gradient (TN, split-K slabs) and the reduction (+ optimiser update) of every gradient
// whose partials are complete before it starts: the weights of layers 1 .. L-1, every bias, the batch normalisations.  One
// kernel, two block ranges, as pair.hip's.  The reduction blocks are memory-latency work (129 and 257 partials per element
// at the contract batch) that depends on nothing the product writes; the product's 512 workgroups of 64 x 64 tiles are two
// per CU where four fit, so the reduction blocks run in the free slots instead of in the launch behind it.
#include "reduce_quad.h"

namespace dcv {

// blocks [0, blocks1): the product, exactly as gemm_kernel<kTN, Cfg, 1, true, false, EpiSlab> runs it (same linear block ->
// (tile, split) map: the slabs come out the same); blocks behind them: reduce_grads_quad_kernel's, on the launch's dynamic LDS
template <class Cfg>
__global__ __launch_bounds__(256, 2) void wgrad_reduce_kernel(Operand A, Operand B, GemmDims d, EpiSlab e, int blocks1, QuadArgs qa,
                                                            float* __restrict__ grads, float* __restrict__ params, float* __restrict__ s1,
                                                            float* __restrict__ s2, float* __restrict__ s3, OptArgs oa) {
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    if ((int)blockIdx.x < blocks1) {
        const BlockMap bm = map_block<kTN>(d, (int)blockIdx.x);
        e.z = bm.split;
        gemm_block<kTN, Cfg, 1, true, false, EpiSlab>(A, B, 0, d, bm.tile_m, bm.tile_n, bm.k_begin, bm.k_end, lds_f, e, -1);
    } else {
        const int b = (int)blockIdx.x - blocks1;
        int l = 0;
        while (l + 1 < qa.n && b >= qa.it[l + 1].blk0) ++l;   // uniform
        const QuadItem& q = qa.it[l];
        double* s_red = reinterpret_cast<double*>(lds_f);
        if (q.groups == 16) reduce_quad_block<16>(q, b - q.blk0, grads, 1.f, 1, params, s1, s2, s3, oa, s_red);
        else reduce_quad_block<4>(q, b - q.blk0, grads, 1.f, 1, params, s1, s2, s3, oa, s_red);
    }
}

template <class Cfg>
static int launch_ride_cfg(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t kc, const EpiSlab& e, const QuadArgs& qa,
                           int64_t qblocks, float* grads, float* params, float* s1, float* s2, float* s3, const OptArgs& oa, hipStream_t s) {
    GemmPlan p;
    const int rc = prepare_gemm<kTN, Cfg, 1, EpiSlab>(A, B, M, N, K, kc, e, nullptr, nullptr, &p);
    if (rc) return rc;
    DCV_REQUIRE(p.vec && !p.gather, "wgrad + reduction launch: operands need the 16-byte, ungathered loader");
    const int64_t blocks1 = (int64_t)p.d.tiles_m * p.d.tiles_n * p.splits;
    DCV_REQUIRE(blocks1 + qblocks < (1ll << 31), "wgrad + reduction launch: grid out of range");
    constexpr size_t lds = gemm_lds_bytes<Cfg, 1>();
    static_assert(lds >= 1024 * sizeof(double), "the reduction blocks take 8 KB of the product's LDS");
    auto kern = wgrad_reduce_kernel<Cfg>;
    if (lds > 64 * 1024) {
        static bool attr_set = false;  // per instantiation
        if (!attr_set) {
            DCV_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            attr_set = true;
        }
    }
    const dim3 grid((unsigned)(blocks1 + qblocks));
    gemm_log_push(kFormRide, kTN, Cfg::TM, Cfg::TN, Cfg::SPLIT, true, false, p.splits, 0);
    if (g_launch_ev.start != nullptr) {   // a profiled launch: the events carry the kernel's own begin / end (common.h)
        const LaunchEvents ev = g_launch_ev;
        g_launch_ev = LaunchEvents{};
        g_launch_taken = ev.start;
        hipExtLaunchKernelGGL(kern, grid, dim3(256), (uint32_t)lds, s, ev.start, ev.stop, 0u, A, B, p.d, e, (int)blocks1, qa, grads, params, s1, s2, s3, oa);
    } else {
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, A, B, p.d, e, (int)blocks1, qa, grads, params, s1, s2, s3, oa);
    }
    DCV_CHECK_LAUNCH();
    return DCV_OK;
}

// the tile families gemm_tn_slab picks for a weight gradient (pick_cfg<kTN>), with the loader of an ungathered batch
bool wgrad_reduce_applies(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t kc) {
    const CfgPick c = pick_cfg<kTN, false>(M, N, K, kc);
    if (c != kPickQuarter && c != kPickBig) return false;
    return A.vec_ok && B.vec_ok && A.rows.idx == nullptr && B.rows.idx == nullptr;
}

int launch_wgrad_reduce(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, int64_t kc, const EpiSlab& e, const QuadArgs& qa,
                        int64_t qblocks, float* grads, float* params, float* s1, float* s2, float* s3, const OptArgs& oa, hipStream_t s) {
    DCV_REQUIRE(wgrad_reduce_applies(A, B, M, N, K, kc) && qblocks > 0, "wgrad + reduction launch: not applicable");
    const bool big = pick_cfg<kTN, false>(M, N, K, kc) == kPickBig;
    if (gemm_split()) {
        if (big) return launch_ride_cfg<CfgBigT<true>>(A, B, M, N, K, kc, e, qa, qblocks, grads, params, s1, s2, s3, oa, s);
        return launch_ride_cfg<CfgQuarterT<true>>(A, B, M, N, K, kc, e, qa, qblocks, grads, params, s1, s2, s3, oa, s);
    }
    if (big) return launch_ride_cfg<CfgBigT<false>>(A, B, M, N, K, kc, e, qa, qblocks, grads, params, s1, s2, s3, oa, s);
    return launch_ride_cfg<CfgQuarterT<false>>(A, B, M, N, K, kc, e, qa, qblocks, grads, params, s1, s2, s3, oa, s);
}

}  // namespace dcv

// Layer forward H = act(X W^T + b): the NT product with the bias / activation / dropout epilogue.
#include "gemm_kernels.h"

namespace dcv {

int gemm_nt_bias_act(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, const EpiBiasAct& epi, hipStream_t s, const TailWs* tw) {
    return launch_gemm<kNT, EpiBiasAct>(A, B, M, N, K, 0, epi, s, nullptr, tw);
}

// the same product as a grouped launch, one member per batch of a validation pass (launch_gemm_group).  In this translation
// unit on purpose: its kernels share the code object the training forward has long loaded when the first pass arrives.
int gemm_nt_bias_act_group(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, const EpiBiasAct& epi, const GroupShift& g, int members,
                           const TailWs* tw, hipStream_t s) {
    return launch_gemm_group<EpiBiasAct>(A, B, M, N, K, epi, g, members, tw, s);
}

}  // namespace dcv

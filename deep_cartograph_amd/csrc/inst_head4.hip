// Layer forward with the fused linear head of up to 4 outputs.
#include "gemm_kernels.h"

namespace dcv {

int gemm_nt_head4(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, const EpiBiasActHead<4>& epi, hipStream_t s, const TailWs* tw) {
    return launch_gemm<kNT, EpiBiasActHead<4>>(A, B, M, N, K, 0, epi, s, nullptr, tw);
}

// the same product as a grouped launch, one member per batch of a validation pass (launch_gemm_group).  In this translation
// unit on purpose: its kernels share the code object the training forward has long loaded when the first pass arrives.
int gemm_nt_head4_group(const Operand& A, const Operand& B, int64_t M, int64_t N, int64_t K, const EpiBiasActHead<4>& epi, const GroupShift& g, int members,
                        const TailWs* tw, hipStream_t s) {
    return launch_gemm_group<EpiBiasActHead<4>>(A, B, M, N, K, epi, g, members, tw, s);
}

}  // namespace dcv

// The persistent decode-layer launch on FP8 weights: fused_block_kernel's one-tile P8
// instantiations (fused_kernels.h, WF = P8: every GEMV stage streams the e4m3 code image of its
// weight, 8 bytes per lane and k-step, and converts each fragment with its row scale in front
// of the MFMA -- bitwise the bf16 kernels on the dequantised weights). A translation unit of
// its own, so that the bf16 kernels in fused.hip compile exactly as they do without it (see
// the note at the top of fused.hip); the launcher stays there.
#include "common.h"

namespace t5g {
T5G_TS_UNIT(fused_p8)
}

#include "fused_kernels.h"

namespace t5g {

// the one-tile P8 kernel for stage S placement sv
fused_block_fn fused_block_p8_kernel(int sv) {
    return sv == 2 ? fused_block_kernel<10> : sv ? fused_block_kernel<9> : fused_block_kernel<8>;
}

}  // namespace t5g

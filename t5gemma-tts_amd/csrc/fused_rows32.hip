// The persistent decode-layer launch for 17-32 rows: fused_block_kernel's two-tile
// instantiations (fused_kernels.h, MT = 2: a second 16-row MFMA tile in every GEMV stage, a norm
// workgroup per two rows, an attention workgroup per (row, kv head)). A translation unit of
// its own, so that the one-tile kernels in fused.hip compile exactly as they do without it
// (see the note at the top of fused.hip); the launcher stays there.
#include "common.h"

namespace t5g {
T5G_TS_UNIT(fused_rows32)
}

#include "fused_kernels.h"

namespace t5g {

// the two-tile kernel for stage S placement sv (0 none, 1 in front, 2 the tail)
fused_block_fn fused_block_rows32_kernel(int sv) {
    return sv == 2 ? fused_block_kernel<6> : sv ? fused_block_kernel<5> : fused_block_kernel<4>;
}

}  // namespace t5g

// The persistent decode-layer launch for 17-32 rows: fused_block_kernel's two-tile
// instantiations (fused.hip, MT = 2: a second 16-row MFMA tile in every GEMV stage, a norm
// workgroup per two rows, an attention workgroup per (row, kv head)). A translation unit of
// its own, so that the one-tile kernels in fused.hip compile exactly as they do without it
// (see the note at the top of fused.hip); the launcher stays there.
#define T5G_FUSED_ROWS32 1
#include "fused.hip"

// The persistent decode-layer launch on FP8 weights: fused_block_kernel's one-tile P8
// instantiations (fused.hip, WF = P8: every GEMV stage streams the e4m3 code image of its
// weight, 8 bytes per lane and k-step, and converts each fragment with its row scale in front
// of the MFMA -- bitwise the bf16 kernels on the dequantised weights). A translation unit of
// its own, so that the bf16 kernels in fused.hip compile exactly as they do without it (see
// the note at the top of fused.hip); the launcher stays there.
#define T5G_FUSED_P8 1
#include "fused.hip"

// The persistent MLP-half decode launch on FP8 weights: fused_mlp_kernel's P8 instantiations
// (fused_kernels.h, V = MT + 8: gate/up and down stream the e4m3 code images, 8 bytes per lane
// and k-step, and convert each fragment with its row scale in front of the MFMA -- bitwise the
// bf16 kernels on the dequantised weights), one tile (1-16 rows) and two (17-32). A translation
// unit of its own, so that every kernel in fused.hip, fused_rows32.hip and fused_p8.hip
// compiles exactly as it does without it (see the note at the top of fused.hip); the launcher
// stays there.
#include "common.h"

namespace t5g {
T5G_TS_UNIT(fused_mlp_p8)
}

#include "fused_kernels.h"

namespace t5g {

typedef void (*fused_mlp_fn)(FusedMlpArgs);

// the P8 MLP-half kernel for MT 16-row tiles
fused_mlp_fn fused_mlp_p8_kernel(int MT) { return MT == 2 ? fused_mlp_kernel<10> : fused_mlp_kernel<9>; }

}  // namespace t5g

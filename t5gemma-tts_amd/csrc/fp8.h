// FP8 weight format "P8" (fp8.hip quantiser, gemv.hip P8 instantiations): OCP e4m3fn codes in
// the lane order of P16 -- fragment (g, kb) = 16 rows x 32 k = 512 bytes, lane l holds
// W[g*16 + (l&15)][kb*32 + 8*(l>>4) + 0..7] as 8 codes -- plus one fp32 scale 2^e per output
// row. 2^e * code is exactly a bf16 number, so a P8 Linear is bitwise the P16 Linear on the
// dequantised weights W_q.
#pragma once
#include "common.h"
#include "t5g_kernels.h"

namespace t5g {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// one lane's 8 codes -> the bf16 A-operand fragment, scaled by the lane's row scale
// (v_cvt_scalef32_pk_bf16_fp8: two codes per convert; exact for power-of-two scales)
__device__ __forceinline__ bf16x8_s p8_to_bf16(u32x2 c, float scale) {
    union {
        bf16x2_b h[4];
        bf16x8_s v;
    } u;
    u.h[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, scale, false);
    u.h[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.x, scale, true);
    u.h[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, scale, false);
    u.h[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c.y, scale, true);
    return u.v;
}

// row groups of a P8 image (not padded to 4 like P16: loads past it return zero codes)
__host__ __device__ inline int p8_groups(int N) { return (N + 15) / 16; }

// fp8.hip: bf16 [N][K] (row stride ld) -> P8 codes, scale[16 * p8_groups(N)] and, unless null,
// the dequantised bf16 [N][K] image; *bad (device) is set when a weight is not finite
int quantize_p8(const bf16_t* src, int N, int K, long ld, uint8_t* p8, float* scale, bf16_t* wq, int* bad,
                hipStream_t st);
// P8 -> row-major bf16 [N][K] through p8_to_bf16
int unpack_p8(const uint8_t* p8, const float* scale, int N, int K, bf16_t* out, hipStream_t st);
// gemv.hip: the register-resident-X GEMV (gemv_rx) on a P8 image: a.W the codes, wscale the
// row scales; a.NG stays the P16 group count (the same units and grid as the bf16 launch)
int gemv_rx_p8(const DecGemmArgs& a, const float* wscale, int epi, hipStream_t st);

}  // namespace t5g

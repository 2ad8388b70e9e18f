// Rounding points of a 64-key decode attention chunk that every placement shares.
//
// The per-op launch (attn.hip attn_decode_kernel + attn_flash_finish), stage S of the layer
// launch (fused_attn.h fb_self_attn) and the layer launch's cross attention (fused_kernels.h stage A)
// must return the same bits. These pieces are the register-only expressions where a result is
// rounded, packed or summed in a fixed order; the sites call them, and each site compiles to
// the machine code it had with the expression written out. The larger steps of a chunk
// (PM-RoPE over a staged row, the score dot, the block sum, P.V, the flash combine's weights)
// stay written out in each kernel: behind a function they change the kernels' schedules and
// measured slower, so the tests keep fencing those.
#pragma once
#include "common.h"

namespace t5g {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// a quad of the projection's summed split-K slabs, rounded to the bf16 tensor the reference's
// projection returns, into the staged q / new key / new value row
__device__ __forceinline__ void stage_round4(float* dst, f32x4 acc) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) dst[jj] = rbf(acc[jj]);
}
// p of the lane's key in a one-chunk row: one aten kv block of `span` keys, the max over the
// wave's scores (s = -inf on lanes without a key), the fast exp or the tail's std::exp by
// position (common.h sdpa_p)
__device__ __forceinline__ float one_block_p(float s, bool live, int lane, int span) {
    const float mx = wave_max(s);
    return live ? sdpa_p(__fsub_rn(s, mx), lane, span) : 0.f;
}
// the four waves' P.V sums of one (head, dimension octet), in wave order
template <int G, int LPK>
__device__ __forceinline__ void fold_ored(f32x4& lo4, f32x4& hi4, const f32x4 (&ored)[4][G][LPK][2], int g, int d8) {
    lo4 = ored[0][g][d8][0] + ored[1][g][d8][0] + ored[2][g][d8][0] + ored[3][g][d8][0];
    hi4 = ored[0][g][d8][1] + ored[1][g][d8][1] + ored[2][g][d8][1] + ored[3][g][d8][1];
}
// the output octet of a one-chunk row: aten scales by the correctly rounded 1 / l, one
// rounding to bf16
__device__ __forceinline__ u32x4 normalise_pack(f32x4 lo4, f32x4 hi4, float l) {
    const float inv = __fdiv_rn(1.0f, l);
    u32x4 w;
    w[0] = pack2(__fmul_rn(lo4[0], inv), __fmul_rn(lo4[1], inv));
    w[1] = pack2(__fmul_rn(lo4[2], inv), __fmul_rn(lo4[3], inv));
    w[2] = pack2(__fmul_rn(hi4[0], inv), __fmul_rn(hi4[1], inv));
    w[3] = pack2(__fmul_rn(hi4[2], inv), __fmul_rn(hi4[3], inv));
    return w;
}
// the output quad of a flash-combined row (fast path: plain 1 / sum, not aten's order)
__device__ __forceinline__ u32x2_t flash_combine_pack(f32x4 acc, float lsum) {
    const float inv = 1.0f / lsum;
    return (u32x2_t){pack2(acc[0] * inv, acc[1] * inv), pack2(acc[2] * inv, acc[3] * inv)};
}

}  // namespace t5g

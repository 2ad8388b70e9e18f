// Norm stages of the persistent decode launches: resid_norm_kernel<4, 2>'s arithmetic on this
// launch's 12 waves (bitwise the per-op launch: tests/test_gpu_fused.py).
#pragma once
#include "fused_sync.h"

namespace t5g {

__device__ __forceinline__ void unpack8f(u32x4 w, float (&v)[8]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = bf_lo(w[j]);
        v[2 * j + 1] = bf_hi(w[j]);
    }
}
__device__ __forceinline__ u32x4 pack8f(const float (&v)[8]) {
    u32x4 w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = pack2(v[2 * j], v[2 * j + 1]);
    return w;
}
// norm.hip's block_sum_once over this launch's 12 waves: the waves past the 288 active
// threads add +0.0f after the 5 real wave sums, which leaves the (non-negative) total
// bitwise unchanged -- the same value as the 288-thread resid_norm launch
__device__ __forceinline__ float fm_block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < FM_NW; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ void fm_rms8(float (&v)[8], bool active, int d, u32x4 w8, float eps, float* red) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
    const float tot = fm_block_sum(active ? ss : 0.f, red);
    const float r = 1.0f / sqrtf(tot / (float)d + eps);
    if (!active) return;
    float wf[8];
    unpack8f(w8, wf);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf((v[j] * r) * (1.0f + wf[j]));
}

// resid_norm_kernel<4, 2>'s arithmetic for row m: v = bf16(sum of the 4 slabs),
// post-norm, h = bf16(r + v) (r8: the residual in, the new residual out, in registers),
// xn = pre-norm(h) stored write-through. Slabs read plain (previous launch) or sc1.
template <int NS, bool SC1>
__device__ __forceinline__ void fb_norm(const float* part, int M, int m, int d, const bf16_t* post_w,
                                        const bf16_t* pre_w, float eps, float (&r8)[8], bf16_t* xn, float* red) {
    const int c = threadIdx.x;
    const bool active = 8 * c < d;
    const int cc = active ? c : d / 8 - 1;
    const u32x4 w_post = *(const u32x4*)(post_w + 8 * cc);
    const u32x4 w_pre = *(const u32x4*)(pre_w + 8 * cc);
    f32x4 p[NS][2];
    const __amdgpu_buffer_rsrc_t pr = raw_rsrc(part, (uint32_t)(NS * M * d * 4));
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int o = ((s * M + m) * d + 8 * cc) * 4;
        if constexpr (SC1) {
            p[s][0] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(pr, o, 0, AUX_SC1));
            p[s][1] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(pr, o + 16, 0, AUX_SC1));
        } else {
            const f32x4* ps = (const f32x4*)(part + ((long)s * M + m) * d + 8 * cc);
            p[s][0] = ps[0];
            p[s][1] = ps[1];
        }
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] += p[s][0][j];
            v[4 + j] += p[s][1][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf(v[j]);
    fm_rms8(v, active, d, w_post, eps, red);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf(r8[j] + v[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) r8[j] = v[j];
    fm_rms8(v, active, d, w_pre, eps, red + 32);
    if (active) {
        const __amdgpu_buffer_rsrc_t xr = raw_rsrc(xn, (uint32_t)(M * d * 2));
        __builtin_amdgcn_raw_buffer_store_b128(pack8f(v), xr, (m * d + 8 * c) * 2, 0, AUX_SC1);
    }
}

// Stage N for row m (resid_norm_kernel<4, 2> with post, resid and pre): xn published sc1.
__device__ __forceinline__ void fm_norm_row(const FusedMlpArgs& a, int m, float* red) {
    const int d = a.d;
    const int c = threadIdx.x;
    const bool active = 8 * c < d;
    const int cc = active ? c : d / 8 - 1;
    const u32x4 w_post = *(const u32x4*)(a.post_w + 8 * cc);
    const u32x4 w_pre = *(const u32x4*)(a.pre_w + 8 * cc);
    const u32x4 rw = *(const u32x4*)(a.h + (long)m * d + 8 * cc);
    f32x4 p[FM_NS][2];
#pragma unroll
    for (int s = 0; s < FM_NS; ++s) {
        const f32x4* ps = (const f32x4*)(a.part_in + ((long)s * a.M + m) * d + 8 * cc);
        p[s][0] = ps[0];
        p[s][1] = ps[1];
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < FM_NS; ++s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] += p[s][0][j];
            v[4 + j] += p[s][1][j];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf(v[j]);
    fm_rms8(v, active, d, w_post, a.eps, red);
    float r8[8];
    unpack8f(rw, r8);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = rbf(r8[j] + v[j]);
    if (active) *(u32x4*)(a.h + (long)m * d + 8 * c) = pack8f(v);   // next launch reads it
    fm_rms8(v, active, d, w_pre, a.eps, red + 32);
    if (active) {
        const __amdgpu_buffer_rsrc_t xr = raw_rsrc(a.xn, (uint32_t)(a.M * d * 2));
        __builtin_amdgcn_raw_buffer_store_b128(pack8f(v), xr, (m * d + 8 * c) * 2, 0, AUX_SC1);
    }
}

}  // namespace t5g

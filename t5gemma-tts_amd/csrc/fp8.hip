// FP8 e4m3 weights for the fast decode step (opt-in): the quantiser bf16 [N][K] -> P8 codes +
// power-of-two row scales + the dequantised bf16 image W_q, and the P8 -> bf16 unpack test
// hook. Layout and convert: fp8.h. Rule per output row: e = the smallest integer >= -100 with
// amax * 2^-e <= 448 (0 for an all-zero row), code = RNE_e4m3fn(w * 2^-e); the NaN codes are
// never produced and 2^e * code is exactly bf16.
#include "../../include/t5gtts.h"
#include "fp8.h"

namespace t5g {

constexpr int P8_EMIN = -100;   // 2^-100 * 2^-9 (the smallest code) is still a normal bf16

// e of a row from its largest finite magnitude: amax = m * 2^x, m in [1, 2): 448 = 1.75 * 2^8
__device__ __forceinline__ int p8_row_exp(float amax) {
    if (amax == 0.f) return 0;
    int ex;
    const float fr = frexpf(amax, &ex);   // amax = fr * 2^ex, fr in [0.5, 1)
    return max(fr <= 0.875f ? ex - 9 : ex - 8, P8_EMIN);
}

// RNE of v (|v| <= 448) to e4m3fn: the code in *code, the rounded value returned
__device__ __forceinline__ float e4m3_rne(float v, uint32_t* code) {
    const float a = fabsf(v);
    int x = -6;   // below the smallest normal 2^-6: subnormal steps of 2^-9
    if (a >= 0.015625f) {
        (void)frexpf(a, &x);
        x -= 1;
    }
    int q = (int)rintf(ldexpf(a, 3 - x));   // 0..16 steps of 2^(x - 3), ties to even
    if (q == 16) {
        q = 8;
        ++x;
    }
    const uint32_t mag = (x == -6 && q < 8) ? (uint32_t)q : (uint32_t)(((x + 7) << 3) | (q - 8));
    *code = ((__float_as_uint(v) >> 24) & 0x80u) | mag;
    return copysignf(ldexpf((float)q, x - 3), v);
}

// one workgroup per 16-row group: the rows' exponents (a wave per row, four at a time), then
// the group's fragments in P16's lane order
__global__ __launch_bounds__(256) void quantize_p8_kernel(const bf16_t* __restrict__ src, int N, int K, long ld,
                                                          uint8_t* __restrict__ p8, float* __restrict__ scale,
                                                          bf16_t* __restrict__ wq, int* bad) {
    __shared__ int es[16];
    const int g = (int)blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int KB = K / 32;
    for (int r = wave; r < 16; r += 4) {
        const long row = (long)g * 16 + r;
        float amax = 0.f;
        if (row < N) {
            for (int k = lane; k < K; k += 64) {
                const bf16_t h = src[row * ld + k];
                if ((h & 0x7f80u) == 0x7f80u) *bad = 1;   // Inf / NaN: the call fails
                else amax = fmaxf(amax, fabsf(bf2f(h)));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        if (lane == 0) {
            const int e = p8_row_exp(amax);
            es[r] = e;
            scale[row] = ldexpf(1.f, e);
        }
    }
    __syncthreads();
    const long row = (long)g * 16 + (lane & 15);
    const int e = es[lane & 15];
    for (int kb = wave; kb < KB; kb += 4) {
        const int k0 = kb * 32 + 8 * (lane >> 4);
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < N) v = *(const u32x4*)(src + row * ld + k0);
        u32x2 c = {0u, 0u};
        u32x4 d = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t h = (v[i >> 1] >> (16 * (i & 1))) & 0xffffu;
            const bool fin = (h & 0x7f80u) != 0x7f80u;
            uint32_t code;
            const float qv = e4m3_rne(fin ? ldexpf(bf2f(h), -e) : 0.f, &code);
            c[i >> 2] |= code << (8 * (i & 3));
            d[i >> 1] |= (uint32_t)f2bf(ldexpf(qv, e)) << (16 * (i & 1));
        }
        *(u32x2*)(p8 + (((long)g * KB + kb) * 64 + lane) * 8) = c;
        if (wq && row < N) *(u32x4*)(wq + row * K + k0) = d;
    }
}

__global__ __launch_bounds__(256) void unpack_p8_kernel(const uint8_t* __restrict__ p8, const float* __restrict__ scale,
                                                        int N, int K, bf16_t* __restrict__ out, int KB, long nfrag) {
    const long frag = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (frag >= nfrag) return;
    const int lane = threadIdx.x & 63;
    const long g = frag / KB;
    const int kb = (int)(frag % KB);
    const long row = g * 16 + (lane & 15);
    if (row >= N) return;
    const u32x2 c = *(const u32x2*)(p8 + (frag * 64 + lane) * 8);
    const bf16x8_s w = p8_to_bf16(c, scale[row]);
    *(bf16x8_s*)(out + row * K + kb * 32 + 8 * (lane >> 4)) = w;
}

int quantize_p8(const bf16_t* src, int N, int K, long ld, uint8_t* p8, float* scale, bf16_t* wq, int* bad,
                hipStream_t st) {
    if (N <= 0 || K <= 0 || K % 32 || ld < K || ld % 8) return -1;
    hipLaunchKernelGGL(quantize_p8_kernel, dim3((unsigned)p8_groups(N)), dim3(256), 0, st, src, N, K, ld, p8, scale,
                       wq, bad);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int unpack_p8(const uint8_t* p8, const float* scale, int N, int K, bf16_t* out, hipStream_t st) {
    if (N <= 0 || K <= 0 || K % 32) return -1;
    const int KB = K / 32;
    const long nfrag = (long)p8_groups(N) * KB;
    hipLaunchKernelGGL(unpack_p8_kernel, dim3((unsigned)((nfrag + 3) / 4)), dim3(256), 0, st, p8, scale, N, K, out, KB,
                       nfrag);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace t5g

using namespace t5g;

extern "C" int64_t t5g_fp8_packed_bytes(int32_t N, int32_t K) {
    if (N <= 0 || K <= 0 || K % 32) return -1;
    return (int64_t)p8_groups(N) * 16 * K;
}

extern "C" int t5g_quantize_weight_fp8(const void* src, int32_t N, int32_t K, int64_t ld, void* p8, float* scale,
                                       void* wq, void* stream) {
    if (!src || !p8 || !scale) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int* bad = nullptr;
    if (hipMalloc(&bad, sizeof(int)) != hipSuccess) return T5G_ENOMEM;
    int rc = hipMemsetAsync(bad, 0, sizeof(int), st) == hipSuccess ? 0 : -2;
    if (!rc) rc = quantize_p8((const bf16_t*)src, N, K, (long)ld, (uint8_t*)p8, scale, (bf16_t*)wq, bad, st);
    int flag = 0;
    if (!rc && (hipMemcpyAsync(&flag, bad, sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess))
        rc = -2;
    (void)hipFree(bad);
    if (rc) return rc == -1 ? T5G_EINVAL : T5G_EHIP;
    return flag ? T5G_EINVAL : T5G_OK;
}

extern "C" int t5g_fp8_unpack(const void* p8, const float* scale, int32_t N, int32_t K, void* out, void* stream) {
    if (!p8 || !scale || !out) return T5G_EINVAL;
    const int rc = unpack_p8((const uint8_t*)p8, scale, N, K, (bf16_t*)out, (hipStream_t)stream);
    return rc == 0 ? T5G_OK : rc == -1 ? T5G_EINVAL : T5G_EHIP;
}

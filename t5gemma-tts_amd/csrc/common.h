// Shared device helpers for the T5Gemma-TTS gfx950 kernels.
// bf16 is carried as raw uint16 bits; all arithmetic is fp32 with explicit
// round-to-nearest-even back to bf16 wherever the reference's bf16 tensor op
// rounds (see DESIGN.md "numerics contract").
#pragma once
#include <hip/hip_runtime.h>

// The in-launch cross-workgroup hand-offs (sampler slice candidates, attention split
// tickets) use the gfx950 form measured valid in the MI355X guide (sc1 write-through
// stores, every storing wave's vmcnt(0) drain, one relaxed agent-scope atomic, sc1
// loads by the last arriver) rather than release/acquire fences. That is a property of
// this ISA's cache policy bits, not of the HIP memory model: refuse any other target.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libt5gtts device code is written for gfx950 (MI355X) only"
#endif
#include <hip/hip_bf16.h>
#include <stdint.h>

typedef uint16_t bf16_t;
typedef short bf16x8_s __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8_b __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define WAVE 64

// Host launchers: function attributes (dynamic LDS opt-in) and device properties are per
// device, so one-time setup is tracked per device, never in a process-global flag (an
// engine per GPU in one process must not skip the second device's setup).
constexpr int T5G_MAX_DEVICES = 64;
static inline int t5g_cur_device() {
    int d = 0;
    return (hipGetDevice(&d) == hipSuccess && d >= 0 && d < T5G_MAX_DEVICES) ? d : -1;
}

__device__ __forceinline__ float bf2f(uint32_t h) { return __uint_as_float(h << 16); }
__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// RNE fp32 -> bf16: gfx950's v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN stays
// NaN), one instruction for two values -- the reference's CPU bf16 casts round the
// same way (torch c10::BFloat16 round_to_nearest_even).
typedef __bf16 bf16x2_b __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
// round an fp32 value to the nearest bf16 value, returned as fp32
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }

__device__ __forceinline__ uint32_t pack2(float a, float b) {
    const bf16x2_b v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, v);
}
// two values rounded to bf16 (one conversion), back as fp32
__device__ __forceinline__ f32x2 rbf2(f32x2 x) {
    const uint32_t w = pack2(x[0], x[1]);
    return (f32x2){__uint_as_float(w << 16), __uint_as_float(w & 0xffff0000u)};
}

// Parity-mode noise: q of one multinomial draw from its two raw MT19937 outputs (hi
// first), as torch's CPU exponential_ (lambda 1) makes it: 53-bit uniform u, then
// -log1p(-u) in double, cast to float, then to bf16 (noise.hip)
__device__ __forceinline__ float mt_exp_q(uint32_t hi, uint32_t lo) {
    const uint64_t r = ((uint64_t)hi << 32) | lo;
    const double u = (double)(r & ((1ull << 53) - 1)) * 0x1.0p-53;
    const double x = -1.0 * log1p(-u);
    return rbf((float)x);
}

// sc1 (write-through store / L1-bypassing load) accessors for in-launch cross-workgroup
// hand-offs (relaxed agent-scope atomics lower to global_store / global_load ... sc1; the
// gfx950 form the file header describes)
template <typename T>
__device__ __forceinline__ void st_sc1(T* p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ T ld_sc1(const T* p) {
    return __hip_atomic_load(const_cast<T*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The value of lane (lane ^ O) for a 32-bit v: the same partner as __shfl_xor(v, O, 64),
// so butterflies built on it add the same pairs in the same order (bit-identical sums),
// but on cheaper paths than ds_bpermute: quad_perm DPP for 1 / 2, row_ror:8 DPP for 8,
// ds_swizzle bit-mode (xor within 32 lanes) for 4 / 16; 32 stays a ds_bpermute.
template <int O>
__device__ __forceinline__ float xlane(float v) {
    static_assert(O == 1 || O == 2 || O == 4 || O == 8 || O == 16 || O == 32, "xor partner");
    if constexpr (O == 1) return __builtin_amdgcn_update_dpp(0.f, v, 0xB1, 0xf, 0xf, false);
    else if constexpr (O == 2) return __builtin_amdgcn_update_dpp(0.f, v, 0x4E, 0xf, 0xf, false);
    else if constexpr (O == 8) return __builtin_amdgcn_update_dpp(0.f, v, 0x128, 0xf, 0xf, false);
    else if constexpr (O == 4 || O == 16)
        return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x1f | (O << 10)));
    else return __shfl_xor(v, 32, 64);
}
template <int O>
__device__ __forceinline__ int xlane(int v) {
    return __float_as_int(xlane<O>(__int_as_float(v)));
}
// argmax step against lane l ^ O: larger value wins, ties to the lower index
template <int O>
__device__ __forceinline__ void xargmax_step(float& v, int& idx) {
    const float ov = xlane<O>(v);
    const int oi = xlane<O>(idx);
    if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
    }
}
__device__ __forceinline__ void wave_argmax(float& v, int& idx) {
    xargmax_step<32>(v, idx);
    xargmax_step<16>(v, idx);
    xargmax_step<8>(v, idx);
    xargmax_step<4>(v, idx);
    xargmax_step<2>(v, idx);
    xargmax_step<1>(v, idx);
}
// butterfly sum over the lanes l ^ {HI/2 ... 1} (HI = a power of two <= 64), largest
// stride first, as `for (o = HI/2; o > 0; o >>= 1) v += __shfl_xor(v, o)`
template <int HI>
__device__ __forceinline__ float xsum(float v) {
    if constexpr (HI >= 64) v += xlane<32>(v);
    if constexpr (HI >= 32) v += xlane<16>(v);
    if constexpr (HI >= 16) v += xlane<8>(v);
    if constexpr (HI >= 8) v += xlane<4>(v);
    if constexpr (HI >= 4) v += xlane<2>(v);
    if constexpr (HI >= 2) v += xlane<1>(v);
    return v;
}

// gfx950 cross-row exchanges on the VALU (v_permlane16/32_swap, no LDS round trip): the value
// of lane l ^ 16 / l ^ 32, as xlane<16> / xlane<32>
__device__ __forceinline__ float xlane16_v(float v) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(((threadIdx.x >> 4) & 1) ? r[0] : r[1]);
}
__device__ __forceinline__ float xlane32_v(float v) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(((threadIdx.x >> 5) & 1) ? r[0] : r[1]);
}
// xsum<HI> (16 <= HI <= 64) with the same adds in the same order and no LDS exchange: the xor-16
// / xor-32 partners through v_permlane*_swap, the xor-4 partner as a 4-lane row rotation (after
// the xor-8 step lanes l and l ^ 8 hold equal values, so lane l + 4 and l - 4 (mod 16) both hold
// lane l ^ 4's value)
template <int HI>
__device__ __forceinline__ float xsum_v(float v) {
    static_assert(HI == 16 || HI == 32 || HI == 64, "butterfly width");
    if constexpr (HI >= 64) v += xlane32_v(v);
    if constexpr (HI >= 32) v += xlane16_v(v);
    v += xlane<8>(v);
    v += __builtin_amdgcn_update_dpp(0.f, v, 0x124, 0xf, 0xf, false);   // row_ror:4
    v += xlane<2>(v);
    v += xlane<1>(v);
    return v;
}

// two xsum_v<32> at once: the sums of a and of b over the lanes of each 32-lane half, a's left
// on the lanes of the even 16-lane rows, b's on the odd rows. One v_permlane16_swap exchanges
// a's odd rows with b's even rows, so the xor-16 step of both butterflies is one add (a lane l
// of an even row: a[l] + a[l ^ 16], of an odd row: b[l ^ 16] + b[l] -- xsum_v's pairs, and
// fp32 addition commutes), and the in-row steps run once instead of twice: bitwise
// xsum_v<32>(a) on the even rows and xsum_v<32>(b) on the odd rows.
__device__ __forceinline__ float xsum2_v32(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    float v = __uint_as_float(r[0]) + __uint_as_float(r[1]);
    v += xlane<8>(v);
    v += __builtin_amdgcn_update_dpp(0.f, v, 0x124, 0xf, 0xf, false);   // row_ror:4
    v += xlane<2>(v);
    v += xlane<1>(v);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    if constexpr (sizeof(T) == 4 && __is_same(T, float)) {
        return xsum<64>(v);
    } else {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
}
// wave64 sum on the DPP network (4 in-row steps, no LDS) + 2 cross-row shuffles; fixed
// order, every lane ends with the total
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_amdgcn_update_dpp(0.f, v, 0xB1, 0xf, 0xf, false);    // quad_perm [1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0.f, v, 0x4E, 0xf, 0xf, false);    // quad_perm [2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0.f, v, 0x141, 0xf, 0xf, false);   // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0.f, v, 0x140, 0xf, 0xf, false);   // row_mirror
    return v;
}
__device__ __forceinline__ float wave_sum_dpp(float v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, xlane<32>(v));
    v = fmaxf(v, xlane<16>(v));
    v = fmaxf(v, xlane<8>(v));
    v = fmaxf(v, xlane<4>(v));
    v = fmaxf(v, xlane<2>(v));
    v = fmaxf(v, xlane<1>(v));
    return v;
}

// block-wide sum for blockDim.x <= 1024; `red` needs 32 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];   // fixed order: deterministic
    return s;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    int nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float s = -INFINITY;
    for (int i = 0; i < nw; ++i) s = fmaxf(s, red[i]);
    return s;
}

// ---- torch CPU SDPA softmax numerics (bf16 inputs), restated bit-exactly -----------
// The reference's attention is F.scaled_dot_product_attention on CPU bf16 tensors
// ([tf] integrations/sdpa_attention.py -> aten cpu_flash_attention, AVX-512 build).
// Per query row and per kv block of <= 512 keys (running max m over the blocks):
//   p_j = exp(s_j - m): the first blen & ~15 keys of the block through at::vec's fast exp
//         (sdpa_fexp, the constants of the shipped kernel), the remaining tail through
//         std::exp(float) = the host's glibc expf (sdpa_expf);
//   tmp_sum = 16 lane accumulators (key % 16, in key order) -> xor 8/4/2/1 tree -> + tail
//         in order (sdpa_block_sum); l = fma(expf(m_old - m), l_old, tmp_sum);
//   out   = bf16(sum_j bf16(p_j) v_j (scaled by expf(m_old - m) per block) * (1 / l)).
// Verified bit-exact against torch 2.10 CPU SDPA in the build container.
__device__ __forceinline__ float sdpa_fexp(float x) {
    if (!(x >= -87.3365478515625f)) return 0.f;           // below ln(FLT_MIN) / masked (-inf)
    const float t = __fmul_rn(x, 1.44269502162933349609375f);   // x * log2(e), fp32 product
    const float n = floorf(t);
    const float f = __fsub_rn(t, n);
    float p = fmaf(f, -0.07920423895120621f, -0.2243383675813675f);
    p = fmaf(f, p, 0.3035426139831543f);
    const float q = fmaf(p, f, 0.00010703434963943437f);
    const float y = fmaf(__fsub_rn(t, q), 8388608.0f, 1065353216.0f);
    return __int_as_float((int)y);                          // cvttps2dq: truncate
}
// std::exp(float) of aten's code = the reference host's glibc 2.35 expf (IFUNC FMA variant
// of sysdeps/ieee754/flt-32/e_expf.c): 2^(k/32) from a 32-entry table times a cubic in r,
// in double with fused multiply-adds. NOT correctly rounded (96 956 inputs of (-87, 0]
// differ), so it is restated operation for operation; oracle/glibc_expf.c is the same
// function, equal to the host's libm on all 2^32 inputs (tools/cpu_order/check_glibc_expf.c).
__device__ __forceinline__ float sdpa_expf(float x) {
    const uint32_t bits = __float_as_uint(x);
    const uint32_t abstop = (bits >> 20) & 0x7ffu;
    if (abstop > 0x42au) {   // |x| >= 88
        if (bits == 0xff800000u) return 0.0f;
        if (abstop > 0x7f7u) return x + x;
        if (x > 0x1.62e42ep6f) return __int_as_float(0x7f800000);
        if (x < -0x1.9fe368p6f) return 0.0f;
        if (x < -0x1.9d1d9ep6f) return 0x1p-149f;
    }
    const double xd = (double)x;
    const double InvLn2N = 0x1.71547652b82fep+5, SHIFT = 0x1.8p+52;
    const double z = __fma_rn(InvLn2N, xd, SHIFT);
    const uint64_t ki = (uint64_t)__double_as_longlong(z);
    const double kd = __dsub_rn(z, SHIFT);
    const double r = __fma_rn(InvLn2N, xd, -kd);
    // 2^(i/32) - (i << 47) table entries (glibc __exp2f_data.tab), i = ki & 31
    uint64_t tb;
    switch ((int)(ki & 31)) {
        case 0: tb = 0x3ff0000000000000ull; break;   case 1: tb = 0x3fefd9b0d3158574ull; break;
        case 2: tb = 0x3fefb5586cf9890full; break;   case 3: tb = 0x3fef9301d0125b51ull; break;
        case 4: tb = 0x3fef72b83c7d517bull; break;   case 5: tb = 0x3fef54873168b9aaull; break;
        case 6: tb = 0x3fef387a6e756238ull; break;   case 7: tb = 0x3fef1e9df51fdee1ull; break;
        case 8: tb = 0x3fef06fe0a31b715ull; break;   case 9: tb = 0x3feef1a7373aa9cbull; break;
        case 10: tb = 0x3feedea64c123422ull; break;  case 11: tb = 0x3feece086061892dull; break;
        case 12: tb = 0x3feebfdad5362a27ull; break;  case 13: tb = 0x3feeb42b569d4f82ull; break;
        case 14: tb = 0x3feeab07dd485429ull; break;  case 15: tb = 0x3feea47eb03a5585ull; break;
        case 16: tb = 0x3feea09e667f3bcdull; break;  case 17: tb = 0x3fee9f75e8ec5f74ull; break;
        case 18: tb = 0x3feea11473eb0187ull; break;  case 19: tb = 0x3feea589994cce13ull; break;
        case 20: tb = 0x3feeace5422aa0dbull; break;  case 21: tb = 0x3feeb737b0cdc5e5ull; break;
        case 22: tb = 0x3feec49182a3f090ull; break;  case 23: tb = 0x3feed503b23e255dull; break;
        case 24: tb = 0x3feee89f995ad3adull; break;  case 25: tb = 0x3feeff76f2fb5e47ull; break;
        case 26: tb = 0x3fef199bdd85529cull; break;  case 27: tb = 0x3fef3720dcef9069ull; break;
        case 28: tb = 0x3fef5818dcfba487ull; break;  case 29: tb = 0x3fef7c97337b9b5full; break;
        case 30: tb = 0x3fefa4afa2a490daull; break;  default: tb = 0x3fefd0765b6e4540ull; break;
    }
    const double s = __longlong_as_double((long long)(tb + (ki << 47)));
    const double p = __fma_rn(r, 0x1.c6af84b912394p-20, 0x1.ebfce50fac4f3p-13);
    const double r2 = __dmul_rn(r, r);
    double y = __fma_rn(r, 0x1.62e42ff0c52d6p-6, 1.0);
    y = __fma_rn(p, r2, y);
    return __double2float_rn(__dmul_rn(y, s));
}
__device__ __forceinline__ float sdpa_exp_tail(float x) { return sdpa_expf(x); }
// p of block position `pos` of a block with `blen` keys
__device__ __forceinline__ float sdpa_p(float x, int pos, int blen) {
    return pos < (blen & ~15) ? sdpa_fexp(x) : sdpa_exp_tail(x);
}
// tmp_sum of one kv block (one wave; every lane returns it). p(pos) -> fp32 p of the
// block's key `pos`, 0 <= pos < blen.
template <typename P>
__device__ __forceinline__ float sdpa_block_sum(int blen, int lane, P p) {
    const int n16 = blen & ~15;
    float acc = 0.f;
    if (lane < 16)
        for (int i = lane; i < n16; i += 16) acc = __fadd_rn(acc, p(i));
    acc = __fadd_rn(acc, xlane<8>(acc));
    acc = __fadd_rn(acc, xlane<4>(acc));
    acc = __fadd_rn(acc, xlane<2>(acc));
    acc = __fadd_rn(acc, xlane<1>(acc));
    float s = __shfl(acc, 0, 64);
    for (int i = n16; i < blen; ++i) s = __fadd_rn(s, p(i));
    return s;
}
// The same tmp_sum from the block's p values already staged in LDS (pl[0, blen); pl must
// hold MAXB + 16 readable floats): every p is computed once, in parallel, by its own
// lane, and only the fixed-order adds are serial. Positions past the block add +0.0f,
// which leaves a sum of non-negative terms bit-unchanged, so the chains are unrolled
// to MAXB without branches. One wave; every lane returns the sum.
template <int MAXB>
__device__ __forceinline__ float sdpa_block_sum_lds(const float* pl, int blen, int lane) {
    const int n16 = blen & ~15;
    const int l16 = lane & 15;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < MAXB / 16; ++k) {
        const int i = l16 + 16 * k;
        acc = __fadd_rn(acc, i < n16 ? pl[i] : 0.f);
    }
    acc = __fadd_rn(acc, xlane<8>(acc));
    acc = __fadd_rn(acc, xlane<4>(acc));
    acc = __fadd_rn(acc, xlane<2>(acc));
    acc = __fadd_rn(acc, xlane<1>(acc));
    float s = __shfl(acc, 0, 64);
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        const int i = n16 + k;
        s = __fadd_rn(s, i < blen ? pl[i] : 0.f);
    }
    return s;
}
// fast-path attention score from the fp32 dot product: x scale, or for an eager
// checkpoint (softcap > 0) the reference's bf16 rounding points of eager_attention_forward
// ([tf] modeling_t5gemma.py:216-221: bf16 q.k, x scale, / softcap, tanh, x softcap)
__device__ __forceinline__ float fast_score(float s, float scale, float softcap) {
    if (softcap > 0.f) {
        const float v = rbf(rbf(s) * scale);
        return rbf(rbf(tanhf(rbf(v / softcap))) * softcap);
    }
    return __fmul_rn(s, scale);
}
// rescale of the previous blocks' sums when the running max grows (std::exp(float) in aten:
// the host's glibc expf, sdpa_expf)
__device__ __forceinline__ float sdpa_block_rescale(float m_old, float m_new) {
    return m_old == -INFINITY ? 0.f : sdpa_expf(__fsub_rn(m_old, m_new));
}
// q-block split of aten's CPU flash attention: a causal query row t of a Tq-query call
// sees keys [0, min(q0 + qsplit, Tk)) in its blocks (keys > t masked), q0 = t - t % qsplit
__device__ __forceinline__ int sdpa_qsplit(int Tq) { return Tq >= 768 ? 256 : (Tq >= 192 ? 64 : 32); }

__device__ __forceinline__ float gelu_tanh(float x) {
    // torch gelu(approximate='tanh') in aten's CPU vector order (no fused multiply-adds):
    // x3 = (x*x)*x; inner = kBeta*(x + kKappa*x3); (0.5*x)*(1 + tanh(inner)); tanh in fp64
    const float k0 = 0.7978845608028654f, k1 = 0.044715f;
    const float x3 = __fmul_rn(__fmul_rn(x, x), x);
    const float inner = __fmul_rn(k0, __fadd_rn(x, __fmul_rn(k1, x3)));
    return __fmul_rn(__fmul_rn(0.5f, x), __fadd_rn(1.f, (float)tanh((double)inner)));
}
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.f + erff(x * 0.7071067811865476f));
}

// Buffer descriptor over one row group's fragment stream: loads past `bytes` return 0
// and move no data (hardware range check), so the weight stream needs no predication.
// Inputs are made provably wave-uniform (readfirstlane) so no waterfall loop appears.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t frag_rsrc(const void* base, uint32_t bytes) {
    const uint64_t p = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
__device__ __forceinline__ bf16x8_s frag_load(__amdgpu_buffer_rsrc_t r, int kb, int lane) {
    // aux 2 = nt: streamed once (decode weights)
    return __builtin_bit_cast(bf16x8_s, __builtin_amdgcn_raw_buffer_load_b128(r, (kb * 64 + lane) * 16, 0, 2));
}

__device__ __forceinline__ f32x4 mfma16(bf16x8_s a, bf16x8_s b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_b, a),
                                                   __builtin_bit_cast(bf16x8_b, b), c, 0, 0, 0);
}

// ---- diagnostic block timelines (built only into the T5G_DBG_TS library variant,
// tools/micro_timeline.cpp): thread 0 of every block stores the 100 MHz device clock
// at numbered points of its kernel, slot 7 = (XCC id << 32) | HW_ID (CU placement).
// Each translation unit has its own buffer pointer, set by t5g_dbg_set_<unit>(); records
// of launch `a.dbg_seq` (args field, 0 in the product) start at block slot dbg_seq * 4096.
#ifdef T5G_DBG_TS
#define T5G_TS_UNIT(unit)                                                          \
    __device__ unsigned long long* t5g_dbg_ts_buf;                                 \
    extern "C" int t5g_dbg_set_##unit(void* p) {                                   \
        return hipMemcpyToSymbol(HIP_SYMBOL(t5g_dbg_ts_buf), &p, sizeof(p)) == hipSuccess ? 0 : -1; \
    }
#define T5G_TS(k)                                                                                  \
    do {                                                                                           \
        if (threadIdx.x == 0 && t5g_dbg_ts_buf) {                                                 \
            const size_t blin_ = (size_t)a.dbg_seq * 4096 +                                         \
                                 blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);   \
            t5g_dbg_ts_buf[blin_ * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                    \
            if ((k) == 0)                                                                          \
                t5g_dbg_ts_buf[blin_ * 8 + 7] =                                                    \
                    ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32) |       \
                    __builtin_amdgcn_s_getreg((31 << 11) | 4);                                     \
        }                                                                                          \
    } while (0)
// the same, stored by thread `tid` (a point reached first by another wave)
#define T5G_TS_BY(k, tid)                                                                          \
    do {                                                                                           \
        if (threadIdx.x == (tid) && t5g_dbg_ts_buf) {                                             \
            const size_t blin_ = (size_t)a.dbg_seq * 4096 +                                         \
                                 blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);   \
            t5g_dbg_ts_buf[blin_ * 8 + (k)] = __builtin_amdgcn_s_memrealtime();                    \
        }                                                                                          \
    } while (0)
// the block-start clock read now, stored later (T5G_TS_START / T5G_TS_COMMIT): a block
// that exits early (a finished sampler row) leaves the previous record intact
#define T5G_TS_START() const unsigned long long t5g_ts0_ = __builtin_amdgcn_s_memrealtime()
#define T5G_TS_COMMIT()                                                                            \
    do {                                                                                           \
        if (threadIdx.x == 0 && t5g_dbg_ts_buf) {                                                 \
            const size_t blin_ = (size_t)a.dbg_seq * 4096 +                                         \
                                 blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);   \
            t5g_dbg_ts_buf[blin_ * 8] = t5g_ts0_;                                                  \
        }                                                                                          \
    } while (0)
#else
#define T5G_TS_UNIT(unit)
#define T5G_TS(k) do { } while (0)
#define T5G_TS_BY(k, tid) do { } while (0)
#define T5G_TS_START() do { } while (0)
#define T5G_TS_COMMIT() do { } while (0)
#endif

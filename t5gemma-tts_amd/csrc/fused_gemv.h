// GEMV stages of the persistent decode launches: gemv_rx_kernel's arithmetic (register-resident
// X, per-wave k-step chains, fixed-order wave reduction), whole (fm_gemv) or split into the
// weight requests (fb_issue) and the rest (fb_finish) so a stage's weights can be requested early.
#pragma once
#include "fp8.h"   // (u32x2: this header stays clear of attn_chunk.h and its u32x2_t, so fused_mlp's sources have no attention header)
#include "fused_sync.h"

namespace t5g {

// The epilogue of a GEMV stage, the one place the bitwise guarantee against the per-op launches
// rests on: the fixed-order reduction of the NWG waves' partial sums (`red`: unit i, tile t at
// (i MT + t) x NWG KiB), then OUT: 0 = GeGLU bf16 (sc1, 8 B), 1 = fp32 plain, 2 = fp32 sc1 (16 B).
template <int NWG, int EPI, int OUT, int MT>
__device__ __forceinline__ void fb_epilogue(int g0, int gs, int nu, int M, void* Y, int ldy, int ybytes, int N,
                                            const f32x4* red) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int xr = lane & 15;
    constexpr bool GLU = EPI == EPI_GEGLU;
    const int n_out = GLU ? N / 2 : N;
    if (wave >= NWG || (MT == 1 && xr >= M) || (GLU && lane >= 32)) return;
    const __amdgpu_buffer_rsrc_t yr = raw_rsrc(Y, (uint32_t)ybytes);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = 16 * t + xr;
        if (MT > 1 && m >= M) continue;
        for (int i = wave; i < nu; i += NWG) {
            const f32x4* ri = red + (size_t)(i * MT + t) * NWG * 64 + lane;
            const int n0 = (g0 + i * gs) * (GLU ? 8 : 16) + 4 * (lane >> 4);
            if constexpr (GLU) {
                f32x4 gsum = {0.f, 0.f, 0.f, 0.f}, usum = gsum;
#pragma unroll
                for (int s2 = 0; s2 < NWG; ++s2) {
                    gsum += ri[s2 * 64];
                    usum += ri[s2 * 64 + 32];
                }
                float v[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = rbf(gelu_tanh(rbf(gsum[r]))) * rbf(usum[r]);
                // act is handed to other workgroups: one 8-byte write-through store
                // (n_out is a multiple of 8 here: fused_mlp checks f % 64)
                const uint2 o2 = {pack2(v[0], v[1]), pack2(v[2], v[3])};
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o2), yr, (m * ldy + n0) * 2, 0, AUX_SC1);
            } else {
                f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s2 = 0; s2 < NWG; ++s2) s4 += ri[s2 * 64];
                if constexpr (OUT == 2) {
                    // n_out is a multiple of 16 here (the q / cross-o widths)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, s4), yr, (m * ldy + n0) * 4, 0,
                                                           AUX_SC1);
                } else {
                    float* y = (float*)Y + (long)m * ldy;   // slabs read by the next launch
                    if (n0 + 3 < n_out) *(f32x4*)(y + n0) = s4;
                    else
                        for (int r = 0; r < 4; ++r)
                            if (n0 + r < n_out) y[n0 + r] = s4[r];
                }
            }
        }
    }
}

// Weight format of a GEMV stage (WF): P16 bf16 fragments, or P8 (fp8.h) --
// e4m3 codes in the same lane order, 8 bytes per lane and k-step, plus the lane's fp32 row
// scale per unit; p8_to_bf16 in front of each MFMA gives exactly the P16 fragment of the
// dequantised weights W_q, so a P8 stage is bitwise the P16 stage on W_q. A stage's weight
// registers FbW<WF, UMAX, SPU>: P16 the fragments, P8 half as many registers for the codes plus
// one scale per unit.
constexpr int WF_P16 = 0, WF_P8 = 1;
template <int WF, int UMAX, int SPU>
struct FbW {
    typedef bf16x8_s frag;   // one lane's registers of a (unit, k-step) fragment
    frag w[UMAX][SPU];
};
template <int UMAX, int SPU>
struct FbW<WF_P8, UMAX, SPU> {
    typedef u32x2 frag;
    frag w[UMAX][SPU];
    float s[UMAX];
};
__device__ __forceinline__ void fb_wload(bf16x8_s& w, __amdgpu_buffer_rsrc_t wr, int off) {
    w = __builtin_bit_cast(bf16x8_s, __builtin_amdgcn_raw_buffer_load_b128(wr, off, 0, AUX_NT));
}
__device__ __forceinline__ void fb_wload(u32x2& w, __amdgpu_buffer_rsrc_t wr, int off) {
    w = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(wr, off, 0, AUX_NT));
}

// One register-resident-X GEMV stage (gemv_rx_kernel's arithmetic): the workgroup's nu
// units g = g0 + i * gs of W (KB k-steps of which [kb_lo, kb_lo + KBs) are summed), X rows from
// `X` (handed off in this launch: sc1 loads), partial sums to LDS `red`, then the
// epilogue. `wait` runs in wave 0 BEFORE its weight requests (the poll must not queue
// behind them); the other waves request their weights first.
// WF = P8 (S: the row scales, null for P16): fb_issue<.., WF_P8>'s requests -- the same (wave,
// unit, k-step) fragments as 8-byte loads from the code image, the lane's row scale once per
// unit -- and each fragment converted in front of the MFMA that takes it, for every tile;
// nothing else differs from the P16 stage.
template <int MT, int EPI, int SPU, int UMAX, int WF = WF_P16, typename Wait, typename Ts>
__device__ __forceinline__ bool fm_gemv(const bf16_t* W, const float* S, int NG, int KB, int kb_lo, int KBs, int g0, int gs,
                                        int nu, const bf16_t* X, int ldx, int xbytes, int M, void* Y, int ldy, int ybytes,
                                        int N, f32x4* red, Wait wait, Ts ts, int ts0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int xr = lane & 15;
    typedef typename FbW<WF, 1, 1>::frag WT;
    constexpr int FB = sizeof(WT);
    const __amdgpu_buffer_rsrc_t wr = frag_rsrc(W, (uint32_t)NG * (uint32_t)KB * (64u * FB));
    auto wbatch = [&](int i, WT(&w)[SPU], float& sc) __attribute__((always_inline)) {
        const int g = g0 + i * gs;
#pragma unroll
        for (int j = 0; j < SPU; ++j) {
            const int kb = wave + j * FM_NW;
            const int off = (i < nu && kb < KBs) ? ((g * KB + kb_lo + kb) * 64 + lane) * FB : (int)0xfffffff0u;
            fb_wload(w[j], wr, off);
        }
        if constexpr (WF == WF_P8) {
            const __amdgpu_buffer_rsrc_t sr = frag_rsrc(S, (uint32_t)NG * 64u);
            sc = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sr, (g * 16 + (lane & 15)) * 4, 0, 0));
        }
    };
    bool ok = true;
    if (wave == 0) ok = wait();
    ts(ts0);
    WT wa[SPU], wb[SPU];
    WT wall[UMAX > 0 ? UMAX : 1][SPU];
    float sa, sb, sall[UMAX > 0 ? UMAX : 1];   // (P8: the lane's row scale of each unit in flight)
    if constexpr (UMAX > 0) {
#pragma unroll
        for (int i = 0; i < UMAX; ++i) wbatch(i, wall[i], sall[i]);
    } else {
        wbatch(0, wa, sa);
    }
    wg_barrier();   // the hand-off is complete (or abandoned) for every wave past here
    // this wave's X fragments: sc1 loads of bytes other workgroups stored sc1
    const __amdgpu_buffer_rsrc_t xrs = raw_rsrc(X, (uint32_t)xbytes);
    bf16x8_s xf[MT][SPU];
    const bf16x8_s z8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int row = 16 * t + xr;
        const int xo = (min(row, M - 1) * ldx + kb_lo * 32 + 8 * (lane >> 4)) * 2;
#pragma unroll
        for (int j = 0; j < SPU; ++j) {
            const int kb = min(wave + j * FM_NW, KBs - 1);
            const bf16x8_s v =
                __builtin_bit_cast(bf16x8_s, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo + kb * 64, 0, AUX_SC1));
            xf[t][j] = (row < M && wave + j * FM_NW < KBs) ? v : z8;
        }
    }
    auto mul = [&](int i, WT(&w)[SPU], float sc) __attribute__((always_inline)) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < SPU; ++j) {
                if constexpr (WF == WF_P8) acc = mfma16(p8_to_bf16(w[j], sc), xf[t][j], acc);
                else acc = mfma16(w[j], xf[t][j], acc);
            }
            if (i < nu) red[((i * MT + t) * FM_NW + wave) * 64 + lane] = acc;
        }
    };
    if constexpr (UMAX > 0) {
#pragma unroll
        for (int i = 0; i < UMAX; ++i) mul(i, wall[i], sall[i]);
    } else {
        for (int i = 0; i < nu; i += 2) {
            wbatch(i + 1, wb, sb);
            mul(i, wa, sa);
            wbatch(i + 2, wa, sa);
            mul(i + 1, wb, sb);
        }
    }
    __syncthreads();
    ts(ts0 + 1);

    constexpr bool GLU = EPI == EPI_GEGLU;
    const int n_out = GLU ? N / 2 : N;
    const __amdgpu_buffer_rsrc_t yr = raw_rsrc(Y, (uint32_t)ybytes);
    if (!(GLU && lane >= 32)) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = 16 * t + xr;
            if (m >= M) continue;
            for (int i = wave; i < nu; i += FM_NW) {
                const f32x4* ri = red + (size_t)(i * MT + t) * FM_NW * 64 + lane;
                const int n0 = (g0 + i * gs) * (GLU ? 8 : 16) + 4 * (lane >> 4);
                if constexpr (GLU) {
                    f32x4 gs = {0.f, 0.f, 0.f, 0.f}, us = gs;
#pragma unroll
                    for (int s2 = 0; s2 < FM_NW; ++s2) {
                        gs += ri[s2 * 64];
                        us += ri[s2 * 64 + 32];
                    }
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = rbf(gelu_tanh(rbf(gs[r]))) * rbf(us[r]);
                    // act is handed to other workgroups: one 8-byte write-through store
                    // (n_out is a multiple of 8 here: fused_mlp checks f % 64)
                    const uint2 o2 = {pack2(v[0], v[1]), pack2(v[2], v[3])};
                    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, o2), yr, (m * ldy + n0) * 2, 0,
                                                          AUX_SC1);
                } else {
                    f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s2 = 0; s2 < FM_NW; ++s2) s4 += ri[s2 * 64];
                    float* y = (float*)Y + (long)m * ldy;   // slabs: read by the next launch
                    if (n0 + 3 < n_out) *(f32x4*)(y + n0) = s4;
                    else
                        for (int r = 0; r < 4; ++r)
                            if (n0 + r < n_out) y[n0 + r] = s4[r];
                }
            }
        }
    }
    return ok;
}

// Split form of fm_gemv: the weight requests (waves < NWG) ...
// One request per (unit, k-step), FB = 16 (P16) or 8 (P8) bytes per lane. P8 (S: the row
// scales): NG is also the image's group count (every width here is a multiple of 16: the
// launcher checks it), so the descriptor ends with the image as gemv_rx_kernel<.., P8>'s does
// and a P16 padding group reads zero codes. The lane's row scale once per unit,
// unconditionally: past the image it reads 0, on zero codes.
template <int NWG, int SPU, int UMAX, int WF = WF_P16>
__device__ __forceinline__ void fb_issue(FbW<WF, UMAX, SPU>& w, const bf16_t* W, const float* S, int NG, int KB,
                                         int kb_lo, int KBs, int g0, int gs, int nu) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= NWG) return;
    constexpr int FB = sizeof(w.w[0][0]);
    const __amdgpu_buffer_rsrc_t wr = frag_rsrc(W, (uint32_t)NG * (uint32_t)KB * (64u * FB));
    // (P16: S is null and sr unused. Built under the `if constexpr` below, the P8 kernels move.)
    const __amdgpu_buffer_rsrc_t sr = frag_rsrc(S, (uint32_t)NG * 64u);
#pragma unroll
    for (int i = 0; i < UMAX; ++i) {
        const int g = g0 + i * gs;
#pragma unroll
        for (int j = 0; j < SPU; ++j) {
            const int kb = wave + j * NWG;
            const int off = (i < nu && kb < KBs) ? ((g * KB + kb_lo + kb) * 64 + lane) * FB : (int)0xfffffff0u;
            fb_wload(w.w[i][j], wr, off);
        }
        if constexpr (WF == WF_P8)
            w.s[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sr, (g * 16 + (lane & 15)) * 4, 0, 0));
    }
}
// ... and the rest: rendezvous, X fragments (sc1), MFMAs, fixed-order wave reduction,
// epilogue. OUT: 0 = GeGLU bf16 (sc1, 8 B), 1 = fp32 plain, 2 = fp32 sc1 (16 B).
// LDSU: units i < nu_reg come from w, unit nu_reg (if < nu) from the LDS image lw (k-steps
// 0 .. NWG * SPU - 1 of one unit, 1 KiB each, fragment layout) -- the same MFMAs in the
// same order as from registers. MT: 16-row MFMA tiles (rows 16 t + lane % 16; every tile takes
// the same weights through the same per-wave k-step chain, its partial sums in its own part of
// `red`: unit i, tile t at (i MT + t) x NWG KiB).
//
// `mid` runs at the split between the two parts -- the MFMA part (rendezvous, X fragments,
// MFMAs, partial sums to `red`, barrier) and the epilogue part (fixed-order reduction,
// epilogue, stores) -- and a wave for which it returns true skips the epilogue: a one-tile
// stage has the waves that store nothing (wave >= nu) request the next stage's weights there.
struct FbNoMid {
    __device__ __forceinline__ bool operator()() const { return false; }
};
//
// WF = P8: each fragment is converted with its unit's row scale (w.s) directly in front of the
// MFMA that takes it -- the MFMA operands are the P16 fragments of W_q in the same order, and
// nothing else differs. The LDS unit is the P8 image too (512 B per k-step, lane-linear: 8
// bytes per lane), converted with w.s[nu_reg], the scale fb_issue loaded for that unit.
template <int NWG, int EPI, int SPU, int UMAX, int OUT, bool LDSU = false, int MT = 1, int WF = WF_P16,
          typename Mid = FbNoMid>
__device__ __forceinline__ void fb_finish(FbW<WF, UMAX, SPU>& w, int g0, int gs, int nu, int kb_lo, int KBs, const bf16_t* X, int ldx, int xbytes, int M, void* Y,
                                          int ldy, int ybytes, int N, f32x4* red, const char* lw = nullptr,
                                          int nu_reg = 0, Mid mid = Mid()) {
    static_assert(MT == 1 || (!LDSU && EPI != EPI_GEGLU), "the LDS unit and the GeGLU epilogue are one-tile only");
    static_assert(WF == WF_P16 || MT == 1, "P8 weights: one tile");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int xr = lane & 15;
    wg_barrier();   // the hand-off is complete (or abandoned) for every wave past here
    if (wave < NWG) {
        const __amdgpu_buffer_rsrc_t xrs = raw_rsrc(X, (uint32_t)xbytes);
        const bf16x8_s z8 = {0, 0, 0, 0, 0, 0, 0, 0};
        const int nr = LDSU ? nu_reg : nu;
        // a tile at a time (its X fragments, then every unit's MFMAs): a stage that holds other
        // requests in flight needs one tile's fragments in registers, not two
        bf16x8_s xf[SPU];
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int row = 16 * t + xr;
            const int xo = (min(row, M - 1) * ldx + kb_lo * 32 + 8 * (lane >> 4)) * 2;
#pragma unroll
            for (int j = 0; j < SPU; ++j) {
                const int kb = min(wave + j * NWG, KBs - 1);
                const bf16x8_s v =
                    __builtin_bit_cast(bf16x8_s, __builtin_amdgcn_raw_buffer_load_b128(xrs, xo + kb * 64, 0, AUX_SC1));
                xf[j] = (row < M && wave + j * NWG < KBs) ? v : z8;
            }
#pragma unroll
            for (int i = 0; i < UMAX; ++i) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < SPU; ++j) {
                    if constexpr (WF == WF_P8) acc = mfma16(p8_to_bf16(w.w[i][j], w.s[i]), xf[j], acc);
                    else acc = mfma16(w.w[i][j], xf[j], acc);
                }
                if (i < nr) red[((i * MT + t) * NWG + wave) * 64 + lane] = acc;
            }
        }
        if constexpr (LDSU) {   // (one tile)
            if (nu_reg < nu) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if constexpr (WF == WF_P8) {
                    float sl = 0.f;   // w.s[nu_reg] without a register-array index
#pragma unroll
                    for (int i = 0; i < UMAX; ++i) sl = i == nu_reg ? w.s[i] : sl;
#pragma unroll
                    for (int j = 0; j < SPU; ++j)
                        acc = mfma16(p8_to_bf16(*(const u32x2*)(lw + ((wave + j * NWG) * 64 + lane) * 8), sl), xf[j], acc);
                } else {
#pragma unroll
                for (int j = 0; j < SPU; ++j)
                    acc = mfma16(*(const bf16x8_s*)(lw + ((wave + j * NWG) * 64 + lane) * 16), xf[j], acc);
                }
                red[(nu_reg * NWG + wave) * 64 + lane] = acc;
            }
        }
    }
    __syncthreads();
    if (mid()) return;
    fb_epilogue<NWG, EPI, OUT, MT>(g0, gs, nu, M, Y, ldy, ybytes, N, red);
}

}  // namespace t5g

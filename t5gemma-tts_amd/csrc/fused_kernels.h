// Decode MLP half of a decoder layer as ONE persistent launch (one workgroup per CU):
//
//   stage N (M workgroups):  h = h + RMSNorm_post(sum of the cross-o slabs); xn = RMSNorm_pre(h)
//   stage G (every workgroup): act = GeGLU(xn . Wgate/up^T)            (gemv_rx_kernel's units)
//   stage D (every workgroup): down slabs[s] = act[:, slice s] . Wdown^T (8 k-slices)
//
// replacing resid_norm_kernel<4,2> + gemv_rx_kernel<12,..,GEGLU> + gemv_rx_kernel<12,..,F32>
// (PMDecoderLayer cross-attention residual + T5GemmaMLP, [tf] modeling_t5gemma.py:81-97,
// hf_export/modeling_t5gemma_voice.py:256-323). What the launch buys is overlap: every
// workgroup requests its whole gate/up weight stream BEFORE the normed rows exist, and its
// down weights before the act slice it multiplies is complete, so the two weight streams
// run back to back while the norm and the hand-offs happen underneath them. Two launch
// boundaries, the norm's launch and the fill / drain of two GEMV launches go away.
//
// Hand-offs between the stages: the sc1 store / drain / barrier / counter recipe, fused_sync.h.
//
// Numerics: every stage is the exact arithmetic of the kernels it replaces (the same
// per-wave k-step chains, the same fixed-order wave reductions, the same norm reductions),
// so the fused launch is bitwise equal to the three launches (tests/test_gpu_fused.py).
//
// Weight formats: the two-tile fused_block_kernel streams bf16 (P16) weights only. The
// one-tile fused_block_kernel also has a P8 form (FP8 e4m3 codes + row scales, fp8.h;
// fused_p8.hip, FusedMlpArgs::wfmt = 1, opt-in through t5g_engine_set_fp8_block): all seven
// weights of a launch as P8 images, 8-byte requests in the places of the 16-byte ones, each
// fragment converted in front of its MFMA -- bitwise the bf16 kernel on the dequantised weights
// (tests/test_gpu_fp8_block.py). fused_mlp_kernel has a P8 form for both tile counts
// (fused_mlp_p8.hip, wfmt = 1 without xattn, opt-in through t5g_engine_set_fp8_mlp): gate/up
// and down as P8 images through fm_gemv<.., WF_P8>, the same requests, hand-offs and sums
// (tests/test_gpu_fp8_mlp.py); the two-tile P8 kernel holds its gate/up units resident, which
// the two-tile bf16 kernel has no registers for.
#pragma once
#include "fused_sync.h"
#include "fused_norm.h"
#include "fused_gemv.h"
#include "fused_attn.h"

namespace t5g {

//
// One template parameter V = MT + 8 WF (MT: 16-row tiles, 1 or 2), so the bf16 kernels keep
// their names fused_mlp_kernel<1> and <2> (bench.py, the profiles and tools/ name them) and their
// code; the P8 kernels are fused_mlp_kernel<9> and <10>.
template <int V>
__global__ __launch_bounds__(FM_NW * 64) void fused_mlp_kernel(FusedMlpArgs a) {
    constexpr int MT = V & 7, WF = V >> 3;
    // gate/up units resident in registers (0: streamed two batches deep). Two tiles of X beside
    // five P16 units do not fit 168 registers; five P8 units (60 codes + 5 scales) do, and are
    // all requested before the N2 wait, as at one tile
    constexpr int UG = (MT == 1 || WF == WF_P8) ? 5 : 0;
    static_assert((MT == 1 || MT == 2) && (WF == WF_P16 || WF == WF_P8), "one or two 16-row tiles, P16 or P8");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* red = (f32x4*)smem;                             // GEMV partial sums
    float* nred = (float*)smem;                            // norm stage: 2 x 32 floats (before the GEMVs)
    unsigned* tmo = a.timeout;
    const int bu = (int)blockIdx.x, nb = (int)gridDim.x;
    const int d = a.d, f = a.f;
    auto ts = [&](int k) __attribute__((always_inline)) { T5G_TS(k); };
    (void)ts;
    T5G_TS(0);
    // the next launch's counters: their last user (the previous step's launch of that
    // layer) has completed, their next user starts after this launch
    if (bu == 0 && threadIdx.x < FM_SET_LINES)
        __hip_atomic_store(a.sync_next + threadIdx.x * FM_LINE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    // ---- stage N: the norm workgroups publish xn rows
    const int nrow = bu - a.norm_b0;
    if (nrow >= 0 && nrow < a.M) {
        fm_norm_row(a, nrow, nred);
        drain_vm();            // every storing wave (R1)
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_fetch_add(a.sync + FS_NORM, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        T5G_TS(1);
    }

    // ---- stage G: a contiguous run of gate/up units (8 act features each). The norm
    // workgroups (the last M) start streaming ~5 us late and take FM_NORM_UNITS units;
    // the others share the rest, the first `uextra` of them one unit more. A run meets at
    // most two down slices.
    const int KBg = d / 32, NGg = a.NGgu;
    const unsigned Mu = (unsigned)a.M;
    constexpr int SPUg = 72 / FM_NW;
    const int nr = nb - a.M, rest = NGg - a.M * FM_NORM_UNITS;
    const int ubase = rest / nr, uextra = rest - ubase * nr;
    const int nu_g = bu < nr ? ubase + (bu < uextra ? 1 : 0) : FM_NORM_UNITS;
    const int g_lo = bu < nr ? bu * ubase + min(bu, uextra) : rest + (bu - nr) * FM_NORM_UNITS;
    bool ok = fm_gemv<MT, EPI_GEGLU, SPUg, UG, WF>(
        a.Wgu, a.sWgu, NGg, KBg, 0, KBg, g_lo, 1, nu_g, a.xn, d, a.M * d * 2, a.M, a.act, f, a.M * f * 2, 2 * f, red,
        [&]() { return fm_wait_n<1>(a.sync, L_N2, Mu, tmo, 1u); }, ts, 2);
    drain_vm();                // act stores of every wave (R1)
    __syncthreads();
    const int units_per_slice = f / FM_DS / 8;   // gate/up units (8 act features each) per down k-slice
    if (threadIdx.x == 0 && nu_g > 0) {   // one arrival per slice the run meets, counting its units
        const int s0 = g_lo / units_per_slice, s1 = (g_lo + nu_g - 1) / units_per_slice;
        for (int sl = s0; sl <= s1; ++sl) {
            const int n = min(g_lo + nu_g, (sl + 1) * units_per_slice) - max(g_lo, sl * units_per_slice);
            __hip_atomic_fetch_add(a.sync + fs_slice(sl), (unsigned)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- stage D: down slice s = bu / dg, units j, j + dg, ... (workgroups past 8 * dg idle)
    const int dg = nb / FM_DS;
    const int s = bu / dg, j = bu - s * dg;
    if (s < FM_DS) {
        const int KBd = f / 32, per = KBd / FM_DS;
        constexpr int SPUd = 36 / FM_NW;
        ok &= fm_gemv<MT, EPI_F32, SPUd, 5, WF>(
            a.Wd, a.sWd, a.NGd, KBd, s * per, per, j, dg, (a.NGd - j + dg - 1) / dg, a.act, f, a.M * f * 2, a.M, a.part_out + (long)s * a.M * d, d,
            0, d, red, [&]() { return fm_wait_n<1>(a.sync, L_SL0 + s, (unsigned)units_per_slice, tmo, 2u + s); }, ts,
            4);
    }
    (void)ok;

    T5G_TS(6);
}

// ===========================================================================
// fused_block_kernel: the cross-attention chain in front of the MLP half (xattn = 1).
//
//   N1 (M norm workgroups)   h1 = h + RMSNorm_post1(o-proj slabs) (kept in registers),
//                            xn1 = RMSNorm_pre1(h1)                       -> L_N1
//   Q  (every workgroup)     one cross-q unit-slice: 16 q columns x 36 k-steps -> L_Q[head]
//   A  (8M workgroups)       PMCrossAttention of (row, q head): q from the 2 slabs, PM-RoPE,
//                            scores / aten softmax / P.V over <= 64 text keys -> L_A[head]
//   O  (every workgroup)     cross-o unit-slices (4 k-slices of 16 k-steps)     -> L_O[wg % 8]
//   N2 (norm workgroups)     h = h1 + RMSNorm_post2(cross-o slabs), xn = RMSNorm_pre2(h) -> L_N2
//   G, D                     as fused_mlp_kernel
//
// replacing resid_norm + cross-q (register-X GEMV, 12 waves, 2 k-slices) + cross attention
// (attn_decode_kernel<256, 1, true>) + cross-o (register-X GEMV, 8 waves, 4 k-slices) in
// front of the three MLP-half launches, with the same arithmetic in every stage (bitwise
// equal to the seven launches: tests/test_gpu_fused.py). Every wave requests the weights
// of a stage as early as its registers allow: Q's before N1 completes, O's during the
// attention, gate/up's right after O (norm workgroups: after N2; one tile: waves 8-10 of the
// workers without an attention task, idle from Q to G, with the LDS copies), down's after gate/up (one
// tile: the waves that store nothing in gate/up's epilogue right after its MFMAs, the storing
// waves after the publish);
// the cross K / V of the attention workgroups and their RoPE table at launch start.
// Round 5 adds the layer's decode self attention as stage S (fb_self_attn, the flash launch's
// arithmetic): fused_block_kernel<1> runs it in front of O1; fused_block_kernel<2> runs the
// NEXT layer's at the end, after the q|k|v stage (its K / V requested before the N3 wait),
// followed by that layer's O1 into the slabs the next launch's N1 reads
// (tests/test_gpu_attn_in_block.py: bitwise equal to the separate flash launch).

// LDS of the attention stage (after the GEMV partial sums)
struct FbAttnLds {
    f32x4 ored[4][32][2];
    float sm[64];
    float pl[64 + 16];
    float qs[256];
    float stat_l;
};
constexpr int FB_D = 2304;                                    // the block kernel's model width
constexpr int FB_GU_KB = FB_D / 32;                           // gate/up k-steps (= FM_NW x 6)
constexpr size_t FB_GU_OFF = (5 * FM_NW * 1024 + sizeof(FbAttnLds) + 16 + 64 * sizeof(float) + FB_D * 2 + 1023) / 1024 * 1024;
constexpr size_t FB_LDS = FB_GU_OFF + (size_t)FB_GU_KB * 1024;
// two 16-row tiles (17-32 rows): the partial sums of both tiles (120 KB; gate/up's 5 units
// stream through registers, no unit in LDS), one attention scratch per q head of the
// workgroup's kv head, the norm scratch and a norm workgroup's two residual rows
constexpr size_t FB_LDS2 = (2 * 5 * FM_NW * 1024 + 2 * sizeof(FbAttnLds) + 16 + 64 * sizeof(float) + 2 * FB_D * 2 + 1023) / 1024 * 1024;

// SM: the self-attention stage S -- 0 none, 1 in front of O1 (a.self_attn), 2 at the end for
// the next layer, followed by the next layer's O1 (a.self_tail; N1 then reads the previous
// launch's o-projection slabs). Separate instantiations, so a launch carries only its own
// stages' code and registers.
//
// MT: 16-row MFMA tiles. MT = 1 serves 1-16 rows, MT = 2 serves 17-32: every GEMV stage
// multiplies each weight fragment into both tiles (fb_finish<.., MT>; gate/up streams its units double-buffered as fused_mlp_kernel<2> does,
// fm_gemv<2>, because five resident units and two tiles of X do not fit 168 registers). The
// worker maps change with it, the per-row arithmetic does not:
//   norms       one workgroup per MT rows, one after the other ((M + 1) / 2 norm workgroups at
//               MT = 2, so nw >= 240 workers and gate/up and down stay at <= 5 units each)
//   attention   MT = 2: one workgroup per (row, kv head), its two q heads side by side on
//               waves 0-3 and 4-7 (32 x 4 = 128 tasks; 32 x 8 (row, q head) tasks would
//               outnumber the workers), each head with the one-head lane map and sums
//   LDS         MT = 2: `red` holds both tiles (120 KB), no gate/up unit in LDS (FB_LDS2);
//               the tail's stage S scratch lives in `red` (free between the q|k|v hand-off
//               and the next layer's O1)
//
// WF: the weight format of every GEMV stage of the launch (all seven weights; no mixed mode).
// WF = P8 (one tile only, fused_p8.hip) streams half the bytes per request and holds half the
// weight registers per stage; the requests (which wave asks for which (unit, k-step), and when:
// O's around the attention, gate/up's with the LDS copies, down's under gate/up's epilogue),
// the hand-offs and every sum are the P16 kernel's. The gate/up unit in LDS is 36 KiB of the
// 72 KiB region; the tail's stage-S scratch keeps its place in that region.
//
// One template parameter V = SM + 4 (MT - 1) + 8 WF, so the bf16 one-tile kernels keep their
// names (fused_block_kernel<0..2>; the profiles and tools/ name them) and their code; the P8
// kernels are fused_block_kernel<8..10>.
template <int V>
__global__ __launch_bounds__(FM_NW * 64) void fused_block_kernel(FusedMlpArgs a) {
    constexpr int SM = V & 3, MT = 1 + ((V >> 2) & 1), WF = V >> 3;
    static_assert(SM <= 2 && (MT == 1 || MT == 2), "S placement 0-2, one or two 16-row tiles");
    static_assert(WF == WF_P16 || (WF == WF_P8 && MT == 1), "P8 weights: the one-tile kernels only");
    constexpr bool SELF = SM == 1;
    constexpr int RED_B = 5 * MT * FM_NW * 1024;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    f32x4* red = (f32x4*)smem;                                   // GEMV partial sums, <= 60 KB per tile
    FbAttnLds* alv = (FbAttnLds*)(smem + RED_B);                 // attention scratch, one per head of the task
    float* nred = (float*)(smem + RED_B + MT * sizeof(FbAttnLds) + 16);   // norm: 2 x 32 floats
    // a norm workgroup's residual rows between N1, N2 and N3 (bf16, exact: every h is rounded)
    u32x4* hrow = (u32x4*)(smem + RED_B + MT * sizeof(FbAttnLds) + 16 + 64 * sizeof(float));
    // a worker's last gate/up unit (72 KiB), fetched by LDS-DMA while the chain runs O1 -> O
    // (one tile only)
    char* gul = smem + FB_GU_OFF;
    unsigned* tmo = a.timeout;
    const int bu = (int)blockIdx.x, nb = (int)gridDim.x;
    const int tq = (int)threadIdx.x, wave = tq >> 6, lane = tq & 63;
    const int d = a.d, f = a.f, M = a.M, D = 256;
    FbAttnLds& al = alv[MT == 2 ? (wave >> 2) & 1 : 0];   // (two tiles: waves 0-3 and 4-7)
    T5G_TS(0);
    if (bu == 0 && tq < FM_SET_LINES)
        __hip_atomic_store(a.sync_next + tq * FM_LINE, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int nn = (M + MT - 1) / MT;   // norm workgroups (MT rows each)
    const int nrow = bu - a.norm_b0;
    const bool normwg = nrow >= 0 && nrow < nn;
    // attention task: (row, q head), or at two tiles (row, kv head) with q head 2 kvh + wave / 4;
    // aw / at: the wave / thread within its head's 4 waves
    const int atasks = MT == 2 ? a.Hkv : a.Hq;
    const bool attnwg = bu < M * atasks;
    const int am = bu / atasks;
    const int ah = MT == 2 ? 2 * (bu - am * atasks) + ((wave >> 2) & 1) : bu - am * atasks;
    const int aw = MT == 2 ? wave & 3 : wave, at = MT == 2 ? tq & 255 : tq;
    bool ok = true;
    // ---- S: the layer's self-attention on every workgroup (O1 waits for its heads)
    if constexpr (SELF) {
        FS_TS(0);
        // a call with more chunk slots than 3 per workgroup: a second pass of 3 nb slots
        // (uniform; two inlined copies -- a loop keeps the stage's registers live across it)
        fb_self_attn<false>(a, *(FbSelfLds*)smem, [] {}, nb, -1, 0);
        if (M * a.Hkv * a.s_nsplit > FS_GRP * nb) fb_self_attn<false>(a, *(FbSelfLds*)smem, [] {}, nb, -1, 1);
        if (FS_DBG_VAR == 4) {   // timing variant: the stage again, warm (points overwritten)
            FS_TS(13);
            fb_self_attn<false>(a, *(FbSelfLds*)smem, [] {}, nb, -1);
        }
        FS_TS(8);
    }
    // the tail's row length, requested first (the oldest load: waiting for it later waits for
    // nothing else); the same slot map as fb_self_attn<true> over the nb - M workers
    int len_tail = 0;
    if constexpr (SM == 2) {
        if (a.Wqkv) FS_TS(0);   // (the last layer's launch has no tail: its start would overwrite)
        const int nwk = nb - nn, cidx = bu + (wave >> 2) * nwk;
        const int rk = cidx % (M * a.Hkv);
        len_tail = a.kv_len[bu < nwk ? rk / a.Hkv : 0];
    }

    // ---- the attention workers request their row's cross K / V chunk and RoPE row
    // (attn_decode_kernel<256, 1, true>'s VFIRST loads, waves 0-3) right after O1
    constexpr int LPK = 32, KPW = 2, KPB = 8, NIT = 8;
    const int kg = lane / LPK, dl = lane % LPK;
    u32x4 kr[NIT], vr[NIT];
    float c8[8], s8[8];
    int alen = 0;
    auto kv_prefetch = [&]() __attribute__((always_inline)) {
    if (attnwg && wave < 4 * MT) {
        alen = a.enc_len[am];
        const int kvc = ah / (a.Hq / a.Hkv);
        const long hs = (long)a.kv_cap * D, bs = hs * a.Hkv;
        const __amdgpu_buffer_rsrc_t krs = frag_rsrc(a.ck + am * bs + kvc * hs, (uint32_t)a.kv_cap * D * 2u);
        const __amdgpu_buffer_rsrc_t vrs = frag_rsrc(a.cv + am * bs + kvc * hs, (uint32_t)a.kv_cap * D * 2u);
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int j = i * KPB + aw * KPW + kg;
            const int off = j < alen ? (j * D + 8 * dl) * 2 : (int)0x7ffffff0;
            kr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, 0, 0));
            vr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrs, off, 0, 0));
        }
        const float* tr = a.rope_tab + (long)am * D + (8 * dl) % (D / 2);
        const f32x4 ca = *(const f32x4*)tr, cb = *(const f32x4*)(tr + 4);
        const f32x4 sa = *(const f32x4*)(tr + D / 2), sb = *(const f32x4*)(tr + D / 2 + 4);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            c8[jj] = ca[jj];
            c8[4 + jj] = cb[jj];
            s8[jj] = sa[jj];
            s8[4 + jj] = sb[jj];
        }
    }
    };

    // ---- the norm workgroups (the last nn): N1, N2, N3 for their rows and nothing else, so no
    // weight stream of their own ever queues ahead of a norm on the critical path
    const int nw = nb - nn;   // GEMV / attention workers
    if (normwg) {
        if constexpr (MT == 1) {
            {
                float hreg[8];
                const int cc = min(tq, d / 8 - 1);
                unpack8f(*(const u32x4*)(a.h + (long)nrow * d + 8 * cc), hreg);
                if (a.Wo1) {   // the o-projection slabs come from this launch's O1 stage
                    if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_P0, (unsigned)(4 * (nw / 4)), tmo, 16u);
                    wg_barrier();
                    fb_norm<FM_NS, true>(a.o1slab, M, nrow, d, a.post1_w, a.pre1_w, a.eps, hreg, a.xn1, nred);
                } else {
                    fb_norm<FM_NS, false>(a.o_slabs, M, nrow, d, a.post1_w, a.pre1_w, a.eps, hreg, a.xn1, nred);
                }
                if (tq < d / 8) hrow[tq] = pack8f(hreg);
                fb_publish(cline(a.sync, L_N1), 1u);
                if constexpr (SELF) FS_TS(12);
            }
            {
                if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_O0, (unsigned)(4 * (nw / 4)), tmo, 4u);
                wg_barrier();
                float r2[8];
                unpack8f(hrow[min(tq, d / 8 - 1)], r2);
                fb_norm<FM_NS, true>(a.oslab, M, nrow, d, a.post_w, a.pre_w, a.eps, r2, a.xn, nred);
                if (tq < d / 8) hrow[tq] = pack8f(r2);
                fb_publish(cline(a.sync, L_N2), 1u);
            }
            {
                if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_D0, (unsigned)(FM_DS * (nw / FM_DS)), tmo, 14u);
                wg_barrier();
                float r3[8];
                unpack8f(hrow[min(tq, d / 8 - 1)], r3);
                fb_norm<FM_DS, true>(a.dslab, M, nrow, d, a.post3_w, a.pre3_w, a.eps, r3, a.xn, nred);
                if (tq < d / 8) *(u32x4*)(a.h + (long)nrow * d + 8 * tq) = pack8f(r3);   // read by the next launch
                fb_publish(cline(a.sync, L_N3), 1u);
            }
            T5G_TS(6);
            return;
        } else {
            // two tiles: this workgroup's rows 2 nrow and 2 nrow + 1 (the last norm workgroup of
            // an odd batch has one), one after the other through the same scratch, one arrival
            // per row. (Its own branch: the one-tile code above stays as it was written.)
            const int r0 = nrow * MT;
            const int nr = min(MT, M - r0);   // rows here, workgroup-uniform
            constexpr int HR = FB_D / 8;      // hrow words per row
            {
                float hreg[MT][8];
                const int cc = min(tq, d / 8 - 1);
#pragma unroll
                for (int t = 0; t < MT; ++t) unpack8f(*(const u32x4*)(a.h + (long)min(r0 + t, M - 1) * d + 8 * cc), hreg[t]);
                if (a.Wo1) {   // the o-projection slabs come from this launch's O1 stage
                    if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_P0, (unsigned)(4 * (nw / 4)), tmo, 16u);
                    wg_barrier();
                }
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    if (t >= nr) continue;
                    if (a.Wo1) fb_norm<FM_NS, true>(a.o1slab, M, r0 + t, d, a.post1_w, a.pre1_w, a.eps, hreg[t], a.xn1, nred);
                    else fb_norm<FM_NS, false>(a.o_slabs, M, r0 + t, d, a.post1_w, a.pre1_w, a.eps, hreg[t], a.xn1, nred);
                    if (tq < d / 8) hrow[t * HR + tq] = pack8f(hreg[t]);
                }
                fb_publish(cline(a.sync, L_N1), (unsigned)nr);
                if constexpr (SELF) FS_TS(12);
            }
            {
                if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_O0, (unsigned)(4 * (nw / 4)), tmo, 4u);
                wg_barrier();
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    if (t >= nr) continue;
                    float r2[8];
                    unpack8f(hrow[t * HR + min(tq, d / 8 - 1)], r2);
                    fb_norm<FM_NS, true>(a.oslab, M, r0 + t, d, a.post_w, a.pre_w, a.eps, r2, a.xn, nred);
                    if (tq < d / 8) hrow[t * HR + tq] = pack8f(r2);
                }
                fb_publish(cline(a.sync, L_N2), (unsigned)nr);
            }
            {
                if (wave == 0) ok &= fm_wait_split<8>(a.sync, L_D0, (unsigned)(FM_DS * (nw / FM_DS)), tmo, 14u);
                wg_barrier();
#pragma unroll
                for (int t = 0; t < MT; ++t) {
                    if (t >= nr) continue;
                    float r3[8];
                    unpack8f(hrow[t * HR + min(tq, d / 8 - 1)], r3);
                    fb_norm<FM_DS, true>(a.dslab, M, r0 + t, d, a.post3_w, a.pre3_w, a.eps, r3, a.xn, nred);
                    if (tq < d / 8) *(u32x4*)(a.h + (long)(r0 + t) * d + 8 * tq) = pack8f(r3);   // read by the next launch
                }
                fb_publish(cline(a.sync, L_N3), (unsigned)nr);
            }
            T5G_TS(6);
            return;
        }
    }
    const int w = bu;   // worker index
    // gate/up: contiguous unit runs over the workers (<= 5 units, the last one from LDS)
    const int KBg = d / 32, NGg = a.NGgu;
    const int ubase = NGg / nw, uextra = NGg - ubase * nw;
    const int nu_g = ubase + (w < uextra ? 1 : 0);
    const int g_lo = w * ubase + min(w, uextra);
    const bool gu_lds = MT == 1 && nu_g > 0 && !attnwg;
    const int oper = nw / 4, so = w / oper, jo = w - so * oper;   // o-projection mapping (O1 and O)
    const bool owork = so < 4;
    const int nu_o = owork ? (a.NGo - jo + oper - 1) / oper : 0;

    // ---- O1: the self-attention o-projection, 4 k-slices of 16 k-steps over nw / 4 workers
    // each (<= 3 units, 8 waves); its input is the previous launch's (no wait), or stage S's:
    // k-slice so is the q-head pair of kv head so, complete when its M rows have published
    if (a.Wo1 && owork) {
        FbW<WF, 3, 2> w1;
        fb_issue<8, 2, 3, WF>(w1, a.Wo1, a.sWo1, a.NGo, a.q_dim / 32, so * 16, 16, jo, oper, nu_o);
        if (SELF && wave == FM_NW - 1) ok &= fm_wait_n<1>(a.sync, L_S0 + so, (unsigned)M, tmo, 17u);
        if constexpr (SELF) FS_TS_BY(9, (FM_NW - 1) * 64);
        fb_finish<8, EPI_F32, 2, 3, 2, false, MT, WF>(w1, jo, oper, nu_o, so * 16, 16, a.att_self, a.q_dim, M * a.q_dim * 2, M,
                                       a.o1slab + (long)so * M * d, d, M * d * 4, d, red);
        fb_publish(cline(a.sync, L_P0 + (w & 7)), 1u);
        if constexpr (SELF) FS_TS(10);
    }
    kv_prefetch();

    // ---- Q: cross-q, 2 k-slices of 36 k-steps over nw / 2 workers each (<= 2 units)
    {
        const int qper = nw / 2, sq = w / qper, jq = w - sq * qper;
        if (sq < 2) {
            const int nu_q = (a.NGq - jq + qper - 1) / qper;
            FbW<WF, 2, 3> wq;
            // every wave's weights first, the poller's too: they were requested ~5 us before
            // N1 completes, so its poll is not held back by them, and wave 0's share no
            // longer starts only when the hand-off is seen
            fb_issue<FM_NW, 3, 2, WF>(wq, a.Wq, a.sWq, a.NGq, d / 32, sq * 36, 36, jq, qper, nu_q);
            if (wave == 0) ok &= fm_wait_n<1>(a.sync, L_N1, (unsigned)M, tmo, 1u);
            T5G_TS(1);
            if constexpr (SELF) FS_TS(11);
            fb_finish<FM_NW, EPI_F32, 3, 2, 2, false, MT, WF>(wq, jq, qper, nu_q, sq * 36, 36, a.xn1, d, M * d * 2, M,
                                               a.qslab + (long)sq * M * a.q_dim, a.q_dim, M * a.q_dim * 4, a.q_dim,
                                               red);
            drain_vm();
            __syncthreads();
            if (tq == 0)
                for (int i = 0; i < nu_q; ++i)
                    __hip_atomic_fetch_add(cline(a.sync, L_Q0 + (jq + i * qper) / (D / 16)), 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // waves 8-10 of the workers that run no attention request the run's last gate/up unit
    // into LDS: 24 x 1 KiB each, no registers, while the attention workers run A (on an
    // attention worker the copies would queue ahead of its q loads). O's publish drains
    // them (vmcnt); its barrier makes them visible to the other waves.
    //
    // The same waves hold nothing else until G (O1, A and O are 8-wave or 4-wave stages), so
    // they request their share of the run's register units (wg: k-steps wave + 12 j) here as
    // well, ~8 us before O's hand-off while HBM is mostly idle, and skip the request at G's
    // entry. g_early is a scalar, so both sides are real branches: these waves cross O on its
    // barriers alone (O's code with wg live is never theirs), and O's publish drains their
    // requests with the LDS copies. Wave 11 polls in O and requests nothing early.
    //
    // P8: the unit is 72 k-steps x 512 B = 36 KiB. LDS-DMA has no 8-byte width, so the copies
    // stay 16 bytes per lane: one instruction moves 1 KiB = two consecutive k-step fragments,
    // 12 per wave. The image is lane-linear, so LDS holds the P8 unit byte for byte (k-step kb
    // at kb x 512, lane l's 8 codes at + 8 l), in the first half of the region.
    FbW<WF, 5, 6> wg;
    const int nu_r = gu_lds ? nu_g - 1 : nu_g;
    const int swave = __builtin_amdgcn_readfirstlane(wave);
    const bool g_early = MT == 1 && gu_lds && swave >= 8 && swave < 11;
    if (gu_lds && wave >= 8 && wave < 11) {
        const int wv = __builtin_amdgcn_readfirstlane(wave - 8);
        if constexpr (WF == WF_P8) {
            constexpr int PER = FB_GU_KB / 2 / 3;   // 1 KiB copies per wave
            const __amdgpu_buffer_rsrc_t gr = frag_rsrc(a.Wgu, (uint32_t)NGg * (uint32_t)KBg * 512u);
            const int gb = (g_lo + nu_g - 1) * KBg * 512 + wv * PER * 1024 + lane * 16;
            __attribute__((address_space(3))) char* dst = (__attribute__((address_space(3))) char*)gul + wv * PER * 1024;
#pragma unroll
            for (int q = 0; q < PER; ++q)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(gr, dst + q * 1024, 16, gb + q * 1024, 0, 0, AUX_NT);
        } else {
        const __amdgpu_buffer_rsrc_t gr = frag_rsrc(a.Wgu, (uint32_t)NGg * (uint32_t)KBg * 1024u);
        const int gb = ((g_lo + nu_g - 1) * KBg + wv * (FB_GU_KB / 3)) * 1024 + lane * 16;
        __attribute__((address_space(3))) char* dst =
            (__attribute__((address_space(3))) char*)gul + wv * (FB_GU_KB / 3) * 1024;
#pragma unroll
        for (int q = 0; q < FB_GU_KB / 3; ++q)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(gr, dst + q * 1024, 16, gb + q * 1024, 0, 0, AUX_NT);
        }
    }
    if (g_early) {
        fb_issue<FM_NW, 6, 5, WF>(wg, a.Wgu, a.sWgu, NGg, KBg, 0, KBg, g_lo, 1, nu_r);
        if (owork) {          // O's rendezvous for a wave with no part in it:
            wg_barrier();     // fb_finish's hand-off barrier,
            __syncthreads();  // the barrier that closes its MFMA part,
            drain_vm();       // and fb_publish (the LDS unit and wg have landed)
            __syncthreads();
        }
    } else {
        // ---- A (attention workers) with O's weight requests around it
        // (two tiles: waves 4-7 run the pair's second head, so O's requests follow the attention)
        FbW<WF, 3, 2> wo;
        if (MT == 1 && attnwg && wave >= 4 && owork) fb_issue<8, 2, 3, WF>(wo, a.Wo, a.sWo, a.NGo, a.q_dim / 32, so * 16, 16, jo, oper, nu_o);
        if (attnwg) {
            const int qcnt = 2 * (D / 16);   // 16 q units per head x 2 k-slices
            // (wave 0's head is the pair's first: two tiles poll both heads' lines at once)
            if (wave == 0) ok &= fm_wait_n<MT>(a.sync, L_Q0 + ah, (unsigned)qcnt, tmo, 2u);
            wg_barrier();
            const int n = alen;
            const int span = alen;
            if (tq < 256 * MT) {
                const int c4 = at < D / 4 ? at : 0;
                const int col = ah * D + 4 * c4;
                const __amdgpu_buffer_rsrc_t qr = raw_rsrc(a.qslab, (uint32_t)(2 * M * a.q_dim * 4));
                const f32x4 u0 = __builtin_bit_cast(
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(qr, (am * a.q_dim + col) * 4, 0, AUX_SC1));
                const f32x4 u1 = __builtin_bit_cast(
                    f32x4, __builtin_amdgcn_raw_buffer_load_b128(qr, ((M + am) * a.q_dim + col) * 4, 0, AUX_SC1));
                const f32x4 acc = u0 + u1;
                if (at < D / 4) {
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) al.qs[4 * c4 + jj] = rbf(acc[jj]);
                }
            }
            fb_lds_barrier();   // LDS only: waves 4-7 keep their O weights in flight
            if (tq < 256 * MT) {
                float q[8];
                const float sg = dl < LPK / 2 ? -1.0f : 1.0f;
                const int pbase = (8 * dl + D / 2) % D;
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const float x = al.qs[8 * dl + jj];
                    const float pr = al.qs[pbase + jj];
                    q[jj] = rbf(rbf(x * c8[jj]) + rbf((sg * pr) * s8[jj]));
                }
#pragma unroll
                for (int i = 0; i < NIT; ++i) {
                    const int j = i * KPB + aw * KPW + kg;
                    if (j >= n) {
                        kr[i] = (u32x4){0u, 0u, 0u, 0u};
                        vr[i] = (u32x4){0u, 0u, 0u, 0u};
                    }
                }
                // every key's reduction before any store (they overlap), exchanges on the VALU
                float scs[NIT];
#pragma unroll
                for (int i = 0; i < NIT; ++i) {
                    float sc = 0.f;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        const float k0 = bf_lo(kr[i][jj]), k1 = bf_hi(kr[i][jj]);
                        sc += q[2 * jj] * k0 + q[2 * jj + 1] * k1;
                    }
                    scs[i] = xsum_v<LPK>(sc);   // xsum<LPK>'s adds
                }
                if (dl == 0) {
#pragma unroll
                    for (int i = 0; i < NIT; ++i) al.sm[i * KPB + aw * KPW + kg] = fast_score(scs[i], a.scale, a.softcap);
                }
            }
            fb_lds_barrier();   // LDS only: waves 4-7 keep their O weights in flight
            if (MT == 1 ? wave == 0 : (wave & ~4) == 0) {   // a head's first wave
                const float sc = lane < n ? al.sm[lane] : -INFINITY;
                const float p = one_block_p(sc, lane < n, lane, span);
                al.pl[lane] = p;
                if (lane < 16) al.pl[64 + lane] = 0.f;
                al.sm[lane] = rbf(p);
                __builtin_amdgcn_wave_barrier();
                const float l = sdpa_block_sum_lds<64>(al.pl, span, lane);
                if (lane == 0) al.stat_l = l;
            }
            fb_lds_barrier();   // LDS only: waves 4-7 keep their O weights in flight
            if (tq < 256 * MT) {
                float o[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) o[jj] = 0.f;
#pragma unroll
                for (int i = 0; i < NIT; ++i) {
                    const int jl = i * KPB + aw * KPW + kg;
                    const float p = al.sm[jl];
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        o[2 * jj] += p * bf_lo(vr[i][jj]);
                        o[2 * jj + 1] += p * bf_hi(vr[i][jj]);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) o[jj] += xlane32_v(o[jj]);   // LPK = 32: one xor-32 step
                if (kg == 0) {
                    al.ored[aw][dl][0] = (f32x4){o[0], o[1], o[2], o[3]};
                    al.ored[aw][dl][1] = (f32x4){o[4], o[5], o[6], o[7]};
                }
            }
            fb_lds_barrier();   // LDS only: waves 4-7 keep their O weights in flight
            if ((MT == 1 ? tq < LPK : (tq & ~256) < LPK) && n > 0) {
                const int d8 = at;
                // (attn_chunk.h fold_ored's order; called here, the two-tile kernels' schedule moves)
                const f32x4 lo4 = al.ored[0][d8][0] + al.ored[1][d8][0] + al.ored[2][d8][0] + al.ored[3][d8][0];
                const f32x4 hi4 = al.ored[0][d8][1] + al.ored[1][d8][1] + al.ored[2][d8][1] + al.ored[3][d8][1];
                const u32x4 w = normalise_pack(lo4, hi4, al.stat_l);
                const __amdgpu_buffer_rsrc_t orr = raw_rsrc(a.att, (uint32_t)(M * a.q_dim * 2));
                __builtin_amdgcn_raw_buffer_store_b128(w, orr, (am * a.q_dim + ah * D + 8 * d8) * 2, 0, AUX_SC1);
            }
            // only a head's first wave stored: it drains and publishes (the other waves' O weight
            // requests stay in flight)
            if (MT == 1 ? wave == 0 : (wave & ~4) == 0) {
                drain_vm();
                if (lane == 0) __hip_atomic_fetch_add(cline(a.sync, L_A0 + ah), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }

        // ---- O: cross-o, 4 k-slices of 16 k-steps over nw / 4 workers each (<= 3 units, 8 waves)
        if (owork) {
            // waves 0-7 (the GEMV) request their weights first; wave 11, idle in this stage and
            // with nothing queued, polls the 8 q heads
            if (!(MT == 1 && attnwg && wave >= 4)) fb_issue<8, 2, 3, WF>(wo, a.Wo, a.sWo, a.NGo, a.q_dim / 32, so * 16, 16, jo, oper, nu_o);
            if (wave == FM_NW - 1) ok &= fm_wait_n<8>(a.sync, L_A0, (unsigned)M, tmo, 3u);
            T5G_TS_BY(2, (FM_NW - 1) * 64);
            fb_finish<8, EPI_F32, 2, 3, 2, false, MT, WF>(wo, jo, oper, nu_o, so * 16, 16, a.att, a.q_dim, M * a.q_dim * 2, M,
                                           a.oslab + (long)so * M * d, d, M * d * 4, d, red);
            fb_publish(cline(a.sync, L_O0 + (w & 7)), 1u);
        }
    }

    // ---- G: gate/up, contiguous unit runs over the workers (<= 5 units; the last from LDS
    // on the workers that fetched it)
    //
    // One tile: a wave that stores nothing in G's epilogue (wave >= nu_g, a scalar so the two
    // sides are real branches) requests its down weights right after G's MFMAs, under the storing
    // waves' epilogue, drain and publish. Only the storing waves drain, and the barrier in front
    // of the publish is the raw one: the early requests stay in flight across it. wg is dead by
    // then, so no two weight arrays are live in any MFMA.
    FbW<WF, 5, 3> wd;
    bool d_early = false;
    if constexpr (MT == 1) {
        if (!g_early) fb_issue<FM_NW, 6, 5, WF>(wg, a.Wgu, a.sWgu, NGg, KBg, 0, KBg, g_lo, 1, nu_r);
        if (wave == 0) ok &= fm_wait_n<1>(a.sync, L_N2, (unsigned)M, tmo, 5u);
        T5G_TS(3);
        const int dper = nw / FM_DS, s = w / dper, j = w - s * dper;   // D's mapping (below)
        d_early = s < FM_DS && __builtin_amdgcn_readfirstlane(wave) >= nu_g;
        fb_finish<FM_NW, EPI_GEGLU, 6, 5, 0, true, 1, WF>(wg, g_lo, 1, nu_g, 0, KBg, a.xn, d, M * d * 2, M, a.act, f,
                                                   M * f * 2, 2 * f, red, gul, nu_r, [&]() {
                                                       if (!d_early) return false;
                                                       const int KBd = f / 32, per = KBd / FM_DS;
                                                       fb_issue<FM_NW, 3, 5, WF>(wd, a.Wd, a.sWd, a.NGd, KBd, s * per, per, j, dper,
                                                                             (a.NGd - j + dper - 1) / dper);
                                                       return true;
                                                   });
        T5G_TS(4);
        if (!d_early) drain_vm();   // act stores of the storing waves (R1)
    } else {
        // two tiles: fused_mlp_kernel<2>'s stage (units streamed two batches deep, both tiles'
        // partial sums in `red`), the first unit requested before the N2 wait
        ok &= fm_gemv<MT, EPI_GEGLU, 6, 0>(
            a.Wgu, nullptr, NGg, KBg, 0, KBg, g_lo, 1, nu_g, a.xn, d, M * d * 2, M, a.act, f, M * f * 2, 2 * f, red,
            [&]() { return fm_wait_n<1>(a.sync, L_N2, (unsigned)M, tmo, 5u); }, [](int) {}, 3);
        T5G_TS(4);
    }
    const int units_per_slice = f / FM_DS / 8;
    if constexpr (MT == 1) {
        wg_barrier();   // every storing wave has drained; the early requests stay in flight
    } else {
        drain_vm();
        __syncthreads();
    }
    if (tq == 0 && nu_g > 0) {
        const int s0 = g_lo / units_per_slice, s1 = (g_lo + nu_g - 1) / units_per_slice;
        for (int sl = s0; sl <= s1; ++sl) {
            const int n = min(g_lo + nu_g, (sl + 1) * units_per_slice) - max(g_lo, sl * units_per_slice);
            __hip_atomic_fetch_add(a.sync + fs_slice(sl), (unsigned)n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    // ---- D: down, 8 k-slices of 36 k-steps over nw / 8 workers each (<= 5 units)
    const int dper = nw / FM_DS, s = w / dper, j = w - s * dper;
    if (s < FM_DS) {
        const int KBd = f / 32, per = KBd / FM_DS;
        const int nu_d = (a.NGd - j + dper - 1) / dper;
        if (!d_early) fb_issue<FM_NW, 3, 5, WF>(wd, a.Wd, a.sWd, a.NGd, KBd, s * per, per, j, dper, nu_d);
        if (wave == 0) ok &= fm_wait_n<1>(a.sync, L_SL0 + s, (unsigned)units_per_slice, tmo, 6u + s);
        T5G_TS(5);
        fb_finish<FM_NW, EPI_F32, 3, 5, 2, false, MT, WF>(wd, j, dper, nu_d, s * per, per, a.act, f, M * f * 2, M,
                                           a.dslab + (long)s * M * d, d, M * d * 4, d, red);
        fb_publish(cline(a.sync, L_D0 + (w & 7)), 1u);
    }

    // ---- QKV: the next layer's q|k|v, 2 k-slices of 36 k-steps over nw / 2 workers each
    // (<= 3 units), weights requested while N3 runs
    if (a.Wqkv) {
        const int kper = nw / 2, sk = w / kper, jk = w - sk * kper;
        if constexpr (SM == 2) {
            // the tail: q|k|v written through and handed off in-launch, the next layer's self
            // attention (its K / V requested before the N3 wait), then the next layer's O1
            const int nu_k = sk < 2 ? (a.NGqkv - jk + kper - 1) / kper : 0;
            FbW<WF, 3, 3> wk;
            fb_issue<FM_NW, 3, 3, WF>(wk, a.Wqkv, a.sWqkv, a.NGqkv, d / 32, sk * 36, 36, jk, kper, nu_k);
            auto mid = [&]() __attribute__((always_inline)) {
                // wave 11 (group 2: never a chunk slot in the tail, so no K / V queued ahead of
                // its polls) waits for N3, then for every q|k|v workgroup
                if (wave == FM_NW - 1) ok &= fm_wait_n<1>(a.sync, L_N3, (unsigned)M, tmo, 15u);
                FS_TS_BY(17, (FM_NW - 1) * 64);
                fb_finish<FM_NW, EPI_F32, 3, 3, 2, false, MT, WF>(wk, jk, kper, nu_k, sk * 36, 36, a.xn, d, M * d * 2, M,
                                                   a.qkv_out + (long)sk * M * a.qkv_dim, a.qkv_dim,
                                                   M * a.qkv_dim * 4, a.qkv_dim, red);
                fb_publish(cline(a.sync, L_K0 + (w & 7)), 1u);   // every worker (an odd one projects nothing)
                FS_TS(18);
                if (wave == FM_NW - 1) ok &= fm_wait_split<8>(a.sync, L_K0, (unsigned)nw, tmo, 19u);
                FS_TS_BY(19, (FM_NW - 1) * 64);
                wg_barrier();
            };
            if constexpr (MT == 1) {
                fb_self_attn<true>(a, *(FbSelfLds*)gul, mid, nw, len_tail);
            } else {
                // two tiles: the q|k|v stage first, then S with its K / V requests (held across
                // the two-tile stage they do not fit the registers: 32 VGPRs spilled, and a
                // request that is spilled has been waited for)
                mid();
                fb_self_attn<true>(a, *(FbSelfLds*)smem, [] {}, nw, len_tail);
            }
            // the next layer's O1: k-slice so waits for kv head so's rows
            if (owork) {
                FbW<WF, 3, 2> w1;
                fb_issue<8, 2, 3, WF>(w1, a.Wo1n, a.sWo1n, a.NGo, a.q_dim / 32, so * 16, 16, jo, oper, nu_o);
                if (wave == FM_NW - 1) ok &= fm_wait_n<1>(a.sync, L_S0 + so, (unsigned)M, tmo, 20u);
                FS_TS_BY(20, (FM_NW - 1) * 64);
                fb_finish<8, EPI_F32, 2, 3, 2, false, MT, WF>(w1, jo, oper, nu_o, so * 16, 16, a.att_self, a.q_dim, M * a.q_dim * 2, M,
                                               a.o1n + (long)so * M * d, d, M * d * 4, d, red);
                FS_TS(21);
            }
        } else if (sk < 2) {
            const int nu_k = (a.NGqkv - jk + kper - 1) / kper;
            FbW<WF, 3, 3> wk;
            fb_issue<FM_NW, 3, 3, WF>(wk, a.Wqkv, a.sWqkv, a.NGqkv, d / 32, sk * 36, 36, jk, kper, nu_k);
            if (wave == 0) ok &= fm_wait_n<1>(a.sync, L_N3, (unsigned)M, tmo, 15u);
            fb_finish<FM_NW, EPI_F32, 3, 3, 1, false, MT, WF>(wk, jk, kper, nu_k, sk * 36, 36, a.xn, d, M * d * 2, M,
                                               a.qkv_out + (long)sk * M * a.qkv_dim, a.qkv_dim, 0, a.qkv_dim, red);
        }
    }
    (void)ok;
    T5G_TS(6);
}

typedef void (*fused_block_fn)(FusedMlpArgs);

}  // namespace t5g

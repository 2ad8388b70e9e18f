// Attention of the persistent decode-layer launch: stage S (the layer's decode self attention,
// fb_self_attn). Stage A, the cross attention of one (row, q head), is inline in
// fused_block_kernel (fused_kernels.h): as functions here it moved the kernels' generated code
// (profiles/fused_split_codegen.txt, step 2e).
#pragma once
#include "attn_chunk.h"
#include "fused_sync.h"

namespace t5g {

// ---- stage S: the layer's decode self-attention (a.self_attn), attn.hip
// attn_decode_kernel<256, 2, true, true> + attn_flash_finish restated on this launch's 12
// waves as three 4-wave groups, each one 64-key chunk in that kernel's lane map: the same
// loads, q / new-key PM-RoPE, cache append, sums and roundings, so the launch stays bitwise
// equal to the flash launch + the per-op chain. Chunk slots (chunk-major: chunk x rows x kv
// heads) run on workgroup c % nwg, group c / nwg, so the K / V stream is spread over every CU. A chunk's partial goes out write-through with one ticket add per
// chunk; the workgroup holding the last chunk of a (row, kv head) combines them in the flash
// kernel's order (its whole workgroup, after every group's ticket) and publishes att_self on
// line L_S0 + kv head, which O1's k-slice of that head pair waits for. Rows of <= 64 keys take
// the kernel's one-block (aten-order) path in their group. Nothing in S waits, so every chunk
// finishes and every (row, kv head) publishes exactly once.
constexpr int FS_G = 2, FS_D = 256, FS_CH = 64, FS_LPK = FS_D / 8, FS_KPW = 64 / FS_LPK, FS_KPB = FS_KPW * 4,
              FS_NIT = FS_CH / FS_KPB, FS_GRP = FM_NW / 4, FS_MAXROWS = 32,
              FS_MAXPASS = 2;   // front: passes of 3 chunk slots per workgroup (8 rows: <= 48 chunks)
static_assert(FS_LPK == 32, "the P.V lanes of a key fold in one xor-32 step");
struct FbSelfGrp {
    f32x4 ored[4][FS_G][FS_LPK][2];
    float sm[FS_G][FS_CH];
    float pl[FS_G][FS_CH + 16];
    float qs[FS_G][FS_D];
    float kvnew[2][FS_D];
    float stat_l[FS_G];
    float cstat[FS_G][2];
    float wts[FS_G][DEC_MAX_CHUNKS];   // the combine's chunk weights and sums
    float lsum[FS_G];
    int last;
};
struct FbSelfLds {
    FbSelfGrp g[FS_GRP];
};
static_assert(sizeof(FbSelfLds) <= 5 * FM_NW * 1024, "stage S lives in the GEMV partial-sum LDS");

// diagnostic timeline of stage S and O1 (T5G_DBG_TS library variant only,
// tools/diag_fused_s.py): thread 0 (or `tid`) of every workgroup stores the 100 MHz clock at
// numbered points, 32 slots per workgroup. The unit that owns the symbols (fs_ts_buf, fs_dbg_var:
// fused.hip) defines T5G_FUSED_DIAG in front of this header; elsewhere the points are empty.
#if defined(T5G_FUSED_DIAG)
#define FS_DBG_VAR fs_dbg_var
#define FS_TS_BY(k, tid)                                                                           \
    do {                                                                                           \
        if (threadIdx.x == (tid) && fs_ts_buf) fs_ts_buf[blockIdx.x * 32 + (k)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define FS_DBG_VAR 0
#define FS_TS_BY(k, tid) do { } while (0)
#endif
#define FS_TS(k) FS_TS_BY(k, 0)

// TAIL (a.self_tail): the stage runs at the END of the previous layer's launch for this
// layer -- the K / V requests go out before `mid` (the N3 wait, the q|k|v stage and its
// hand-off, run by the caller), the q|k|v slabs are read (sc1) after it; slots live on the
// first `nwg` workgroups' groups 0-1 only (group 2's waves poll), and `len_in` is the row
// length the caller requested at launch start. Front: `mid` is empty, len_in < 0.
template <bool TAIL, typename Mid>
__device__ __forceinline__ void fb_self_attn(const FusedMlpArgs& a, FbSelfLds& sl, Mid&& mid, int nwg, int len_in,
                                             int pass = 0) {
    constexpr int G = FS_G, D = FS_D, LPK = FS_LPK, KPW = FS_KPW, KPB = FS_KPB, NIT = FS_NIT;
    const int tq = (int)threadIdx.x, wave = tq >> 6, lane = tq & 63;
    // (tail: the group and with it the slot's row geometry are wave-uniform, held in scalar
    // registers across `mid`)
    const int grp = TAIL ? __builtin_amdgcn_readfirstlane(wave >> 2) : wave >> 2, gw = wave & 3, gt = tq & 255;
    const int kg = lane / LPK, dl = lane % LPK;
    const int M = a.M, Hkv = a.Hkv;
    FbSelfGrp& L = sl.g[grp];
    // this group's chunk slot (row m, kv head, chunk sp): slot c = sp x (M Hkv) + row x Hkv +
    // kv head on workgroup c % nb, group c / nb -- known before the row lengths, so the q|k|v
    // slabs and the RoPE row are requested with the row length; chunk-major, so the live
    // chunks (sp < the row's count) fill group 0 of every workgroup before any group 1
    // (in front, a call with more slots than 3 nb runs several passes: slots 3 nb p ..)
    const int cidx = (int)blockIdx.x + (grp + FS_GRP * pass) * nwg;
    const bool has_s = (int)blockIdx.x < nwg && cidx < M * Hkv * a.s_nsplit;
    const int sp = has_s ? cidx / (M * Hkv) : 0, rk = has_s ? cidx - sp * (M * Hkv) : 0;
    const int m = rk / Hkv, kvh = rk - m * Hkv;
    const int dvar = FS_DBG_VAR;
    const int len = TAIL ? __builtin_amdgcn_readfirstlane(len_in) : a.kv_len[m];
    int role = 0, c4 = 0, g_own = 0, col;
    if (gt < G * D / 4) {
        g_own = gt / (D / 4);
        c4 = gt % (D / 4);
        col = (kvh * G + g_own) * D + 4 * c4;
    } else {   // the appended key / value (used by the slot holding key t)
        const int idx = gt - G * D / 4;
        role = 1 + idx / (D / 4);   // 1: key, 2: value
        c4 = idx % (D / 4);
        col = (role == 1 ? a.q_dim : a.q_dim + Hkv * D) + kvh * D + 4 * c4;
    }
    const long uo = dvar == 2 ? 0 : col;
    // unconditional (slots past the grid read row 0's): a load under a branch makes the
    // compiler wait for everything in flight at the join, the row length included. In the
    // tail the slabs are this launch's (after `mid`).
    f32x4 u0, u1;
    if constexpr (!TAIL) {
        u0 = *(const f32x4*)(a.qkv_in + (long)m * a.qkv_dim + uo);
        u1 = *(const f32x4*)(a.qkv_in + ((long)M + m) * a.qkv_dim + uo);
    }
    const float* tr = a.rope_tab + (long)m * D + (8 * dl) % (D / 2);
    f32x4 ca = *(const f32x4*)tr, cb = *(const f32x4*)(tr + 4);
    f32x4 sa = *(const f32x4*)(tr + D / 2), sb = *(const f32x4*)(tr + D / 2 + 4);
    // row geometry (attn_decode_kernel's rules: causal, the sliding window); a row of <= 64
    // keys is one chunk (the one-block path; a row with no key still publishes)
    const int t = len - 1;
    const int hi = min(t + 1, len), lo = a.window > 0 ? max(0, t - a.window + 1) : 0;
    const int span = max(hi - lo, 0);
    const bool single = span <= FS_CH;
    const int nch = single ? 1 : (span + FS_CH - 1) / FS_CH;
    const bool has_c = has_s && sp < nch;
    if (has_s && sp == 0 && gt == 0 && nch > a.s_nsplit)   // past the host's key bound: give every wait up
        __hip_atomic_store(a.timeout, 18u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int c0 = lo + sp * FS_CH, c1 = min(hi, c0 + FS_CH), n = c1 - c0;
    const bool gv = has_c && n > 0;
    const bool has_t = gv && t >= c0 && t < c1;
    if (!TAIL && gt == 0) L.last = 0;
    const __amdgpu_buffer_rsrc_t ors = raw_rsrc(a.att_self, (uint32_t)(M * a.q_dim * 2));
    const long nrec = (long)M * Hkv * a.s_nsplit;
    const __amdgpu_buffer_rsrc_t prs = frag_rsrc(a.fpart, (uint32_t)(nrec * G * D * 4));
    const __amdgpu_buffer_rsrc_t srs = frag_rsrc(a.fstat, (uint32_t)(nrec * G * 2 * 4));
    const long hs = (long)a.s_cap * D, bs = hs * Hkv;
    bf16_t* Kb = a.sk + (dvar == 3 ? 0 : m * bs + kvh * hs);
    bf16_t* Vb = a.sv + (dvar == 3 ? 0 : m * bs + kvh * hs);
    float c8[8], s8[8];
    const __amdgpu_buffer_rsrc_t krs = frag_rsrc(Kb, (uint32_t)a.s_cap * D * 2u);
    const __amdgpu_buffer_rsrc_t vrs = frag_rsrc(Vb, (uint32_t)a.s_cap * D * 2u);
    // groups without a chunk request nothing (a wave-uniform branch): their loads would queue
    // in the CU's memory pipeline ahead of the working groups' data
    u32x4 kr[NIT], vr[NIT];
    if (gv && dvar != 5) {
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int j = c0 + i * KPB + gw * KPW + kg;
            const int off = (j < c1 && dvar != 1) ? (j * D + 8 * dl) * 2 : (int)0x7ffffff0;
            kr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(krs, off, 0, 0));
            vr[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(vrs, off, 0, 0));
        }
        // q (and the appended key / value) staged in the same block as the K / V requests, so
        // the wait for the slabs counts exactly the requests behind them
        if constexpr (!TAIL) {
            f32x4 acc = u0;
            acc += u1;
            if (role == 0) stage_round4(&L.qs[g_own][4 * c4], acc);
            else if (has_t) stage_round4(&L.kvnew[role - 1][4 * c4], acc);
        }
        // the RoPE row consumed here too (an empty asm use): past the branch join the compiler
        // would otherwise wait for nearly every K / V request before the q rotation
        asm volatile("" : "+v"(ca), "+v"(cb), "+v"(sa), "+v"(sb));
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            c8[jj] = ca[jj];
            c8[4 + jj] = cb[jj];
            s8[jj] = sa[jj];
            s8[4 + jj] = sb[jj];
        }
    } else {
#pragma unroll
        for (int i = 0; i < NIT; ++i) kr[i] = vr[i] = (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) c8[jj] = s8[jj] = 0.f;
    }
    if constexpr (TAIL) {
        mid();   // N3, the q|k|v stage and its hand-off (workgroup-uniform, with barriers)
        const __amdgpu_buffer_rsrc_t qrs = raw_rsrc(a.qkv_in, (uint32_t)(2 * M * a.qkv_dim * 4));
        u0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(qrs, (int)((m * a.qkv_dim + uo) * 4), 0, AUX_SC1));
        u1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(qrs, (int)(((M + m) * a.qkv_dim + uo) * 4), 0,
                                                                              AUX_SC1));
        if (gt == 0) L.last = 0;
        if (gv) {
            f32x4 acc = u0;
            acc += u1;
            if (role == 0) stage_round4(&L.qs[g_own][4 * c4], acc);
            else if (has_t) stage_round4(&L.kvnew[role - 1][4 * c4], acc);
        }
    }
    fb_lds_barrier();
    FS_TS(2);
    // groups without a chunk skip the arithmetic too (wave-uniform): their waves would take
    // VALU issue slots from the working groups on the same SIMDs
    if (gv) {
        float q[G][8];
        {
            const float sg = dl < LPK / 2 ? -1.0f : 1.0f;
            const int pbase = (8 * dl + D / 2) % D;
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) {
                    const float x = L.qs[g][8 * dl + jj];
                    const float pr = L.qs[g][pbase + jj];
                    q[g][jj] = rbf(rbf(x * c8[jj]) + rbf((sg * pr) * s8[jj]));
                }
        }
        FS_TS(14);
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            // (keys past c1 were requested out of the descriptor's range: already zero)
            const int j = c0 + i * KPB + gw * KPW + kg;
            if (has_t && j == t) {
                // key t: PM-RoPE of the new key, then append it and its value
                const float sg = dl < LPK / 2 ? -1.0f : 1.0f;
                const int pbase = (8 * dl + D / 2) % D;
                u32x4 kw, vw;
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    float ko[2], vo[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int dd = 8 * dl + 2 * jj + e;
                        const float c = c8[2 * jj + e], sn = s8[2 * jj + e];
                        const float x = L.kvnew[0][dd], pr = L.kvnew[0][pbase + 2 * jj + e];
                        ko[e] = rbf(rbf(x * c) + rbf((sg * pr) * sn));
                        vo[e] = L.kvnew[1][dd];
                    }
                    kw[jj] = pack2(ko[0], ko[1]);
                    vw[jj] = pack2(vo[0], vo[1]);
                }
                kr[i] = kw;
                vr[i] = vw;
                *(u32x4*)(Kb + (long)t * D + 8 * dl) = kw;
                *(u32x4*)(Vb + (long)t * D + 8 * dl) = vw;
            }
        }
        // the scores stay in registers until every key's reduction is done (no store between
        // them), so the 16 butterfly reductions of a wave overlap instead of running one by one
        // the two q heads side by side in packed fp32 (v_pk_mul / v_pk_add: the same IEEE
        // operations per head, half the instructions)
        static_assert(G == 2, "packed head pair");
        f32x2 qq[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) qq[jj] = (f32x2){q[0][jj], q[1][jj]};
        // a key's two heads reduced together (common.h xsum2_v32: one cross-row swap and one
        // set of in-row steps for both, the same adds as xsum_v<LPK> per head): head 0's score
        // lands on the lanes of the even 16-lane rows, head 1's on the odd rows
        float sc[NIT];
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            f32x2 s2 = {0.f, 0.f};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const float k0 = bf_lo(kr[i][jj]), k1 = bf_hi(kr[i][jj]);
                s2 += qq[2 * jj] * k0 + qq[2 * jj + 1] * k1;
            }
            sc[i] = xsum2_v32(s2[0], s2[1]);   // xsum<LPK>'s adds, VALU exchanges
        }
        FS_TS(16);
        if (dl % 16 == 0) {
            const int g = dl / 16;
#pragma unroll
            for (int i = 0; i < NIT; ++i) L.sm[g][i * KPB + gw * KPW + kg] = fast_score(sc[i], a.scale, a.softcap);
        }
    }
    fb_lds_barrier();
    FS_TS(3);
    // softmax of the chunk: one aten block (one-block row) or the flash chunk statistics
    if (gv && gw < G) {
        const int g = gw;
        const float s = lane < n ? L.sm[g][lane] : -INFINITY;
        const float mx = wave_max(s);
        if (single) {
            const float p = lane < n ? sdpa_p(__fsub_rn(s, mx), lane, span) : 0.f;   // (attn_chunk.h one_block_p; mx is the flash branch's too)
            L.pl[g][lane] = p;
            if (lane < 16) L.pl[g][FS_CH + lane] = 0.f;
            L.sm[g][lane] = rbf(p);
            __builtin_amdgcn_wave_barrier();
            const float l = sdpa_block_sum_lds<FS_CH>(L.pl[g], span, lane);
            if (lane == 0) L.stat_l[g] = l;
        } else {
            const float p = lane < n ? __expf(s - mx) : 0.f;
            L.sm[g][lane] = rbf(p);
            const float l = xsum<64>(p);
            if (lane == 0) {
                L.cstat[g][0] = mx;
                L.cstat[g][1] = l;
            }
        }
    }
    fb_lds_barrier();
    if (gv) {
        // both heads' accumulators packed (o2[d] = {head 0, head 1}): the same per-head chain
        f32x2 o2[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) o2[jj] = (f32x2){0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NIT; ++i) {
            const int jl = i * KPB + gw * KPW + kg;
            const f32x2 pp = {L.sm[0][jl], L.sm[1][jl]};
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                o2[2 * jj] += pp * bf_lo(vr[i][jj]);
                o2[2 * jj + 1] += pp * bf_hi(vr[i][jj]);
            }
        }
        float o[G][8];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) o[g][jj] = o2[jj][g] + xlane32_v(o2[jj][g]);   // LPK = 32: one xor-32 step
        if (kg == 0) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                L.ored[gw][g][dl][0] = (f32x4){o[g][0], o[g][1], o[g][2], o[g][3]};
                L.ored[gw][g][dl][1] = (f32x4){o[g][4], o[g][5], o[g][6], o[g][7]};
            }
        }
    }
    fb_lds_barrier();
    FS_TS(4);
    if (gv && gt < G * LPK) {
        const int g = gt / LPK, d8 = gt % LPK;
        f32x4 lo4, hi4;
        fold_ored<G, LPK>(lo4, hi4, L.ored, g, d8);
        if (single) {   // the row's output
            const u32x4 w = normalise_pack(lo4, hi4, L.stat_l[g]);
            __builtin_amdgcn_raw_buffer_store_b128(w, ors, (m * a.q_dim + (kvh * G + g) * D + 8 * d8) * 2, 0, AUX_SC1);
        } else {        // the chunk's partial
            const int off = (int)(((((long)m * Hkv + kvh) * a.s_nsplit + sp) * G + g) * D + 8 * d8) * 4;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, lo4), prs, off, 0, AUX_SC1);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, hi4), prs, off + 16, 0, AUX_SC1);
        }
    }
    if (gv && !single && gt < G) {
        const u32x2_t st = {__float_as_uint(L.cstat[gt][0]), __float_as_uint(L.cstat[gt][1])};
        __builtin_amdgcn_raw_buffer_store_b64(
            st, srs, (int)(((((long)m * Hkv + kvh) * a.s_nsplit + sp) * G + gt) * 2) * 4, 0, AUX_SC1);
    }
    drain_vm();
    fb_lds_barrier();
    FS_TS(5);
    unsigned* tk = a.fticket + (long)m * Hkv + kvh;
    if (has_c && !single && gt == 0)
        L.last = __hip_atomic_fetch_add(tk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(nch - 1);
    fb_lds_barrier();
    FS_TS(6);
    // the group holding the last chunk of its (row, kv head) combines the chunk records
    // (attn_flash_finish's combine on the group's 4 waves: waves 0..G-1 the chunk weights
    // exp(m_c - M) and the sum, waves G.. the output quads, their first batch of partials
    // requested before the weights are known); every group that completed a (row, kv head)
    // then publishes it. The groups of a workgroup combine side by side.
    const bool comb = has_c && !single && L.last != 0;
    const bool pub = has_c && (single || comb);
    {
        constexpr int FB = 16, NOUT = G * D / 4;   // attn_flash_finish's combine batch
        const long rec = ((long)m * Hkv + kvh) * a.s_nsplit;   // chunk records of this (row, kv head)
        const int ot = gt - 64 * G;
        const bool outer = comb && ot >= 0 && ot < NOUT;
        const int og = outer ? ot / (D / 4) : 0, o4 = outer ? ot % (D / 4) : 0;
        auto pload = [&](f32x4 (&pv)[FB], int cb) {
#pragma unroll
            for (int k = 0; k < FB; ++k) {
                int off = cb + k < nch ? (int)((((rec + cb + k) * G + og) * D + 4 * o4) * 4) : (int)0x7ffffff0;
                asm volatile("" : "+v"(off));
                pv[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, off, 0, AUX_SC1));
            }
        };
        if (comb && gt == 0) __hip_atomic_store(tk, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        f32x4 pv[FB];
        if (outer) pload(pv, 0);
        if (comb && gw < G) {
            constexpr int CPL = DEC_MAX_CHUNKS / 64;   // lane owns chunks lane + 64 i (attn_flash_finish)
            const int g = gw;
            float mc[CPL], lc[CPL];
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int c = lane + 64 * i;
                int off = c < nch ? (int)((((rec + c) * G + g) * 2) * 4) : (int)0x7ffffff0;
                asm volatile("" : "+v"(off));
                const u32x2_t st = __builtin_amdgcn_raw_buffer_load_b64(srs, off, 0, AUX_SC1);
                mc[i] = c < nch ? __uint_as_float(st[0]) : -INFINITY;
                lc[i] = c < nch ? __uint_as_float(st[1]) : 0.f;
            }
            float mm = mc[0];
#pragma unroll
            for (int i = 1; i < CPL; ++i) mm = fmaxf(mm, mc[i]);
            const float Mx = wave_max(mm);
            float wl = 0.f;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const float w = lane + 64 * i < nch ? __expf(mc[i] - Mx) : 0.f;
                L.wts[g][lane + 64 * i] = w;
                wl += w * lc[i];
            }
            const float Ls = xsum<64>(wl);
            if (lane == 0) L.lsum[g] = Ls;
        }
        fb_lds_barrier();
        if (outer) {   // attn_flash_finish's batches of 16 records, in order
            f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int cb = 0; cb < nch; cb += FB) {
                if (cb > 0) pload(pv, cb);
#pragma unroll
                for (int k = 0; k < FB; ++k) {
                    const float w = cb + k < nch ? L.wts[og][cb + k] : 0.f;
                    acc += w * pv[k];
                }
            }
            const u32x2_t ow = flash_combine_pack(acc, L.lsum[og]);
            __builtin_amdgcn_raw_buffer_store_b64(ow, ors, (m * a.q_dim + (kvh * G + og) * D + 4 * o4) * 2, 0,
                                                  AUX_SC1);
        }
    }
    drain_vm();
    fb_lds_barrier();
    if (pub && gt == 0) __hip_atomic_fetch_add(cline(a.sync, L_S0 + kvh), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    FS_TS(7);
}

}  // namespace t5g

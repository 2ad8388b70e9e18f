// Outside the product path: the hipEvent timing hooks (t5g_time_*; bench.py --full prices its
// rooflines with them, tools/ probe with them) and the stand-alone op wrappers tests and probes
// call (t5g_gemm, t5g_gemv, t5g_resid_norm(_src), t5g_rope_store, the attention and exact-order
// entry points, ...).
// The decode hooks launch what a decode step launches: they take the step's plan
// (decode_plan, engine.hip) instead of deciding for themselves.
#include <algorithm>

#include "engine_state.h"
#include "fp8.h"

// Mean microseconds of n calls of body(i) -> T5G code, between two events recorded on st
// around the calls (warm-up launches belong before this). The events are destroyed on every
// path; a failing body ends the loop and its code is returned.
namespace {
struct EventPair {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~EventPair() {
        for (hipEvent_t x : ev)
            if (x) hipEventDestroy(x);
    }
};
}   // namespace
template <typename F>
static int time_loop(hipStream_t st, int n, F body, float* avg_us) {
    EventPair p;
    for (hipEvent_t& x : p.ev) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(p.ev[0], st));
    for (int i = 0; i < n; ++i) {
        const int rc = body(i);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(p.ev[1], st));
    HIPCHK(hipEventSynchronize(p.ev[1]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.ev[0], p.ev[1]));
    *avg_us = ms * 1000.f / (float)n;
    return T5G_OK;
}

// a persistent launch's code as the hooks report it (-1: not built for these args / this device)
static int launch_rc(int rc) { return rc == 0 ? T5G_OK : rc == -1 ? T5G_EUNSUPPORTED : T5G_EHIP; }

// diagnostic T5G_TIME_SHARE (tools/probe_cache_share.py): 1 "chain" -- every launch reads
// layer 1's projection weights and cross K / V (they then stay in the Infinity Cache; the
// gate/up and down weights rotate); 2 "gd" -- layer 1's gate/up and down (the rest rotates):
// which bytes' cache residency a persistent launch is sensitive to
static int time_share() {
    const char* s = getenv("T5G_TIME_SHARE");
    return !s ? 0 : !strcmp(s, "chain") ? 1 : !strcmp(s, "gd") ? 2 : 0;
}

extern "C" int t5g_mt_stream(const uint32_t* init, int32_t B, int64_t n_out, int64_t out_stride, uint32_t* out,
                             int64_t snap_every, int32_t n_snap, uint32_t* snap, void* stream) {
    RC(mt_stream(init, B, (long)n_out, (long)out_stride, out, (long)snap_every, n_snap, snap, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_sdpa_expf(const float* x, float* y, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && (!x || !y))) return T5G_EINVAL;
    RC(sdpa_expf_array(x, y, (long)n, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_mt_exponential(const uint32_t* raw, int64_t n, void* q, void* stream) {
    RC(mt_exponential(raw, (long)n, (bf16_t*)q, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_sort_emu_wave(int32_t n, int32_t S, int32_t* pos_dev, float* val_dev, int32_t* tag_dev,
                                 int32_t* fail_dev, void* stream) {
    RC(sort_emu_wave(n, S, pos_dev, val_dev, tag_dev, fail_dev, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_gemm(const void* X, int32_t ldx, int32_t M, const void* Wp, int32_t N, int32_t K, int32_t splits,
                        const void* bias, void* Y, int32_t ldy, int32_t epi, void* stream) {
    if (!X || !Wp || !Y || M <= 0 || N <= 0 || K % 32) return T5G_EINVAL;
    const bool prefill = (epi & T5G_GEMM_PREFILL) != 0, pf_reg = (epi & T5G_GEMM_PREFILL_REG) != 0;
    RC(gemm((const bf16_t*)X, ldx, M, Wp, N, K, splits, bias, Y, ldy, epi & 0xff, (hipStream_t)stream, prefill,
            pf_reg));
    return T5G_OK;
}

extern "C" int t5g_time_gemm(const void* X, int32_t ldx, int32_t M, const void* const* Wp_list, int32_t n_w,
                             int32_t N, int32_t K, int32_t splits, void* Y, int32_t ldy, int32_t epi, int32_t iters,
                             void* stream, float* avg_us) {
    if (iters <= 0 || !avg_us || !Wp_list || n_w <= 0) return T5G_EINVAL;
    for (int i = 0; i < n_w; ++i)
        if (!Wp_list[i]) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool pf = (epi & T5G_GEMM_PREFILL) != 0, pf_reg = (epi & T5G_GEMM_PREFILL_REG) != 0;
    epi &= 0xff;
    auto launch = [&](int i) -> int {
        RC(gemm((const bf16_t*)X, ldx, M, Wp_list[i % n_w], N, K, splits, nullptr, Y, ldy, epi, st, pf, pf_reg));
        return T5G_OK;
    };
    if (const int rc = launch(0)) return rc;   // warm
    return time_loop(st, iters, launch, avg_us);
}

extern "C" int t5g_time_decode_step(t5g_engine* e, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || e->B <= 0) return T5G_EINVAL;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const int rc = time_loop(st, iters, [&](int) { return decode_forward(e, st); }, avg_us);
    return rc ? rc : check_handoff(e, st);
}

// hipEvent-timed exact decode Linears (parity mode's dominant kernel, xmm_dec_kernel): per
// iteration the six launches of one decoder layer as the parity decode step runs them --
// q|k|v, o, cross-q, cross-o (bf16 out), gate/up (GeGLU epilogue), down (K parts) -- on
// the decode X16 buffers of B rows, layers rotated so every launch streams from HBM.
// Average microseconds per layer (six launches) in *avg_us.
extern "C" int t5g_time_exact_linears(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || B <= 0 || B > e->c.max_batch || !e->exact || !e->xmm_ready) return T5G_EINVAL;
    e->decode_state_invalid = true;
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate;
    hipStream_t st = (hipStream_t)stream;
    auto layer = [&](int l) -> int {
        const t5g_engine::XLayer& X = e->dec_x[l];
        RC(xlin16(e, e->dxn16, B, X.qkv, e->qkv_dim, d, nullptr, e->qkv, e->qkv_dim, nullptr, EPI_BF16, nullptr,
                  nullptr, e->q_dim, e->kv_dim, e->q_dim, st));
        RC(xlin16(e, e->datt16, B, X.o, d, e->q_dim, nullptr, e->tmp, d, nullptr, EPI_BF16, nullptr, nullptr, d, 0, 0,
                  st));
        RC(xlin16(e, e->dxn16, B, X.cross_q, e->q_dim, d, nullptr, e->dq, e->q_dim, nullptr, EPI_BF16, nullptr,
                  nullptr, e->q_dim, 0, 0, st));
        RC(xlin16(e, e->datt16, B, X.cross_o, d, e->q_dim, nullptr, e->tmp, d, nullptr, EPI_BF16, nullptr, nullptr, d,
                  0, 0, st));
        RC(xlin16(e, e->dxn16, B, X.gate_up, 2 * f, d, nullptr, nullptr, f, e->dact16, EPI_GEGLU, nullptr, nullptr, f,
                  0, 0, st));
        int np = 0;
        RC(xlin16_dec_parts(e, e->dact16, B, X.down, d, f, e->tmp, d, nullptr, &np, st));
        return T5G_OK;
    };
    if (const int rc = layer(0)) return rc;   // untimed: the first launch's one-time setup
    return time_loop(st, iters, [&](int i) { return layer(i % c.n_dec_layers); }, avg_us);
}

// hipEvent-timed parity-mode persistent layer launches (xlayer.hip; bench.py parity roofline):
// whole rotations over the layers as a decode step runs them (layer l's counter set zeroed by
// layer l - 1's launch), one untimed rotation first, on the engine's current decode state
extern "C" int t5g_time_xlayer(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || B <= 0 || B > e->c.max_batch || !e->exact || !e->xmm_ready) return T5G_EINVAL;
    if (!xlayer_usable(e, B)) return T5G_EUNSUPPORTED;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const int L = e->c.n_dec_layers;
    const int n = (iters + L - 1) / L * L;
    for (int l = 0; l < L; ++l)
        if (const int rc = launch_rc(xlayer_launch(xlayer_args(e, B, l), st))) return rc;
    const int share = time_share();
    const XLayerArgs a1 = xlayer_args(e, B, 1);
    auto launch = [&](int i) {
        XLayerArgs a = xlayer_args(e, B, i % L);
        if (share == 1 && a.Wqkv) {
            a.Wo = a1.Wo, a.Wq = a1.Wq, a.Wco = a1.Wco, a.Wqkv = a1.Wqkv, a.ck = a1.ck, a.cv = a1.cv;
        } else if (share == 2) {
            a.Wgu = a1.Wgu, a.Wd = a1.Wd;
        }
        return launch_rc(xlayer_launch(a, st));
    };
    const int rc = time_loop(st, n, launch, avg_us);
    return rc ? rc : check_handoff(e, st);
}

// hipEvent-timed fused decode-MLP launches (bench.py roofline leg): layers rotated, so every
// launch streams its weights from HBM (2.2 GB of gate/up + down > the 256 MiB Infinity Cache)
extern "C" int t5g_time_decode_mlp(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || B <= 0 || B > e->c.max_batch || e->c.n_dec_layers < 2) return T5G_EINVAL;
    // FP8 mode: only with t5g_engine_set_fp8_mlp on (fused_args then carries the P8 images)
    if (e->fp8 && !e->fp8_mlp) return T5G_EUNSUPPORTED;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const int L = e->c.n_dec_layers;
    // whole rotations over the layers, as a decode step runs them: layer l's launch finds
    // its counter set zeroed by layer l - 1's (the last launch before this call was a step's
    // last layer, which zeroed layer 0's set); one untimed rotation first
    const int n = (iters + L - 1) / L * L;
    // the launch a decode step runs at B rows, by the step's plan with the hook's own row
    // limit: the whole-layer launch (without stage S) up to 16 rows when the device supports
    // it, the MLP half alone otherwise. As before the plan existed, the hook does not ask
    // t5g_engine_set_fused (switches false) and lets layer 0's check stand for every layer.
    const DecodePlan p = decode_plan(e, B, 16, false);
    const bool block = p.block && fused_mlp_check(fused_block_args(e, B, 0)) == 0;
    auto launch = [&](int i) {
        return launch_rc(fused_mlp(block ? fused_block_args(e, B, i % L) : fused_args(e, B, i % L), st));
    };
    for (int l = 0; l < L; ++l)
        if (const int rc = launch(l)) return rc;
    const int rc = time_loop(st, n, launch, avg_us);
    return rc ? rc : check_handoff(e, st);   // a timed launch that gave up would report a false rate
}

// hipEvent-timed persistent layer launches WITH the self-attention stage S, as the fast
// decode step runs them (bench.py roofline leg): whole rotations over the layers at the
// cache lengths the last call left (each launch re-appends its rows' last key and value, the
// values the slabs in e->part give). *keys = the keys one launch reads per kv head, summed
// over the rows and averaged over the layers (sliding layers clipped to their window).
extern "C" int t5g_time_decode_layer(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us,
                                     float* keys) {
    if (!e || iters <= 0 || !avg_us || !keys || B <= 0 || B > e->c.max_batch || e->c.n_dec_layers < 2) return T5G_EINVAL;
    // FP8 mode: only with t5g_engine_set_fp8_block on (the plan below then refuses > 16 rows)
    if (e->fp8 && !e->fp8_block) return T5G_EUNSUPPORTED;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const t5g_config& c = e->c;
    const int L = c.n_dec_layers;
    // attn_in_block 1: launch l runs layer l's attention in front; 2: layer l + 1's at its end
    // (the last launch none; layer 0's is the step's own launch, not timed here); mode 2 on a
    // call the tail does not take runs S in front. All of it is the decode step's plan, with
    // the hook's own row limit (it times the one-tile launch: past 16 rows bench.py prices the
    // MLP-half launch). As before the plan existed, the hook does not ask t5g_engine_set_fused
    // or, for the tail, t5g_engine_set_attn_flash (switches false).
    const DecodePlan p = decode_plan(e, B, 16, false);
    if (!p.block) return T5G_EUNSUPPORTED;
    const bool tail = p.tail;
    auto args = [&](int l, FusedMlpArgs& fa) {
        if (!tail) return decode_layer_launch(e, p, B, l, fa) == DL_BLOCK_S;
        fa = fused_block_args(e, B, l);
        return fused_block_tail(e, l, fa);
    };
    FusedMlpArgs fa;
    for (int l = 0; l < L; ++l)
        if (!args(l, fa)) return T5G_EUNSUPPORTED;
    std::vector<int> len(B);
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(len.data(), e->kv_len, sizeof(int) * B, hipMemcpyDeviceToHost));
    double ksum = 0.0;
    for (int l = tail ? 1 : 0; l < L; ++l)
        for (int b = 0; b < B; ++b) {
            const int w = c.dec_sliding[l] ? c.sliding_window : 0;
            ksum += w > 0 ? std::min(len[b], w) : len[b];
        }
    *keys = (float)(ksum / L);
    const int n = (iters + L - 1) / L * L;
    // T5G_TIME_SHARE: each launch keeps its own layer's hand-off counter sets, so the
    // synchronisation is the decode step's (a launch repeating a layer would find its counters
    // un-zeroed)
    const int share = time_share();
    FusedMlpArgs f1;
    if (share && !args(1, f1)) return T5G_EUNSUPPORTED;
    for (int l = 0; l < L; ++l)
        if (const int rc = args(l, fa) ? launch_rc(fused_mlp(fa, st)) : T5G_EUNSUPPORTED) return rc;
    auto launch = [&](int i) -> int {
        if (!args(i % L, fa)) return T5G_EUNSUPPORTED;
        if (share == 1 && i % L != L - 1) {
            fa.Wq = f1.Wq, fa.Wo = f1.Wo, fa.Wqkv = f1.Wqkv, fa.ck = f1.ck, fa.cv = f1.cv;
            fa.sWq = f1.sWq, fa.sWo = f1.sWo, fa.sWqkv = f1.sWqkv;   // (P8: a weight's scales go with it)
            if (fa.Wo1n) fa.Wo1n = f1.Wo1n, fa.sWo1n = f1.sWo1n;
        } else if (share == 2) {
            fa.Wgu = f1.Wgu, fa.Wd = f1.Wd;
            fa.sWgu = f1.sWgu, fa.sWd = f1.sWd;
        }
        return launch_rc(fused_mlp(fa, st));
    };
    const int rc = time_loop(st, n, launch, avg_us);
    return rc ? rc : check_handoff(e, st);
}

// work = scores | chunk maxima (fp32)
// work of t5g_attention_decode(_flash), in 4-byte words: scores | chunk maxima | flash
// partials | flash chunk stats | flash tickets (last, so one zeroing covers them)
struct AttnWork {
    int64_t sc, mx, fp, fs, tk;
};
static AttnWork attn_work_layout(int B, int Hq, int Hkv, int D, int cap) {
    const int64_t nsplit = (cap + 63) / 64, G = Hq / Hkv;
    AttnWork w;
    w.sc = (int64_t)B * Hq * cap;
    w.mx = (int64_t)B * Hkv * nsplit * G;
    w.fp = (int64_t)B * Hkv * nsplit * G * D;
    w.fs = (int64_t)B * Hkv * nsplit * G * 2;
    w.tk = (int64_t)B * Hkv;
    return w;
}

extern "C" int64_t t5g_attention_decode_work_bytes(int32_t B, int32_t Hq, int32_t Hkv, int32_t D, int32_t cap) {
    if (B <= 0 || Hkv <= 0 || Hq % Hkv || D <= 0 || cap <= 0) return -1;
    const AttnWork w = attn_work_layout(B, Hq, Hkv, D, cap);
    return (w.sc + w.mx + w.fp + w.fs + w.tk) * 4;
}

static int attention_decode_abi(const t5g_attn_decode_args* g, bool flash, void* stream);
extern "C" int t5g_attention_decode(const t5g_attn_decode_args* g, void* stream) {
    return attention_decode_abi(g, false, stream);
}
extern "C" int t5g_attention_decode_flash(const t5g_attn_decode_args* g, void* stream) {
    return attention_decode_abi(g, true, stream);
}

static int attention_decode_abi(const t5g_attn_decode_args* g, bool flash, void* stream) {
    if (!g || !g->q || !g->k_cache || !g->v_cache || !g->kv_len || !g->out || !g->work) return T5G_EINVAL;
    if (g->B <= 0 || g->n_kv_heads <= 0 || g->n_heads % g->n_kv_heads || g->cap <= 0 ||
        g->cap > SDPA_KV_BLOCK * SDPA_MAX_BLOCKS || !(g->softcap >= 0.f && g->softcap < INFINITY))   // negative, NaN or infinite
        return T5G_EINVAL;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = (const bf16_t*)g->q;
    a.ldq = g->n_heads * g->head_dim;
    a.Mq = g->B;
    a.K = (const bf16_t*)g->k_cache;
    a.V = (const bf16_t*)g->v_cache;
    a.kv_hstride = (long)g->cap * g->head_dim;
    a.kv_bstride = a.kv_hstride * g->n_kv_heads;
    a.kv_len = g->kv_len;
    a.Hkv = g->n_kv_heads;
    a.D = g->head_dim;
    a.G = g->n_heads / g->n_kv_heads;
    a.causal = g->causal;
    a.window = g->window;
    a.scale = g->scale;
    a.softcap = g->softcap;   // the score of common.h fast_score; a.eager stays 0 (that is attn_kernel's variant)
    a.O = (bf16_t*)g->out;
    a.ldo = a.ldq;
    a.chunk = 64;
    a.nsplit = (g->cap + 63) / 64;
    a.kv_cap = g->cap;
    const AttnWork w = attn_work_layout(g->B, g->n_heads, g->n_kv_heads, g->head_dim, g->cap);
    a.sbuf = (float*)g->work;
    a.mbuf = a.sbuf + w.sc;
    a.flash = flash ? 1 : 0;
    a.fpart = a.mbuf + w.mx;
    a.fstat = a.fpart + w.fp;
    a.fticket = (unsigned*)(a.fstat + w.fs);
    RC(attention_decode(a, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_resid_norm(int32_t M, int32_t d, const void* delta, const void* resid, const void* post_w,
                              const void* pre_w, float eps, void* resid_out, void* normed_out, void* stream) {
    if (M <= 0 || d <= 0 || d % 8 || !delta || !resid_out) return T5G_EINVAL;
    NormArgs n = norm_args(M, d, eps);
    n.delta = (const bf16_t*)delta;
    n.resid = (const bf16_t*)resid;
    n.post_w = (const bf16_t*)post_w;
    n.pre_w = (const bf16_t*)pre_w;
    n.resid_out = (bf16_t*)resid_out;
    n.normed_out = (bf16_t*)normed_out;
    RC(resid_norm(n, (hipStream_t)stream));
    return T5G_OK;
}

static_assert(sizeof(t5g_norm_src_args) == 136, "t5g_norm_src_args layout");

extern "C" int t5g_resid_norm_src(const t5g_norm_src_args* g, void* stream) {
    if (!g || g->M <= 0 || g->d <= 0 || g->d % 8 || g->d > 8 * 1024) return T5G_EINVAL;
    if ((g->delta != nullptr) + (g->ids != nullptr) + (g->part != nullptr) != 1) return T5G_EINVAL;
    if (g->ids && (!g->table || g->n_table <= 0)) return T5G_EINVAL;
    if (g->part && (g->nsplit < 1 || g->nsplit > 8 || g->ldp < g->d || g->ldp % 4)) return T5G_EINVAL;
    if ((!g->resid_out && !g->normed_out) || (g->pre_w && !g->normed_out)) return T5G_EINVAL;
    if (g->rope_tab && (!g->rope_pos || !g->rope_inv_freq || g->rope_D <= 0 || g->rope_D % 2)) return T5G_EINVAL;
    // out_rows: the slabs' row stride is M (the compact count), and without resid or delta
    // resid_norm()'s stand-in for the absent resid is a compact output buffer, which the kernel
    // reads at the source row -- past its end. resid_norm() itself does not check this (its
    // engine caller gathers with delta); a caller that adds another out_rows form must.
    if (g->out_rows && g->part) return T5G_EUNSUPPORTED;
    if (g->out_rows && !g->resid && !g->delta) return T5G_EINVAL;
    NormArgs n = norm_args(g->M, g->d, g->eps);
    n.delta = (const bf16_t*)g->delta;
    n.ids = g->ids;
    n.table = (const bf16_t*)g->table;
    n.n_table = g->n_table;
    n.scale = g->scale;
    n.part = g->part;
    n.nsplit = g->part ? g->nsplit : 0;
    n.ldp = g->ldp;
    n.resid = (const bf16_t*)g->resid;
    n.post_w = (const bf16_t*)g->post_w;
    n.pre_w = (const bf16_t*)g->pre_w;
    n.resid_out = (bf16_t*)g->resid_out;
    n.normed_out = (bf16_t*)g->normed_out;
    n.out_rows = g->out_rows;
    if (g->rope_tab) {
        n.rope_pos = g->rope_pos;
        n.rope_inv_freq = g->rope_inv_freq;
        n.rope_tab = g->rope_tab;
        n.rope_D = g->rope_D;
    }
    RC(resid_norm(n, (hipStream_t)stream));
    return T5G_OK;
}

static_assert(sizeof(t5g_rope_store_args) == 152, "t5g_rope_store_args layout");

extern "C" int t5g_rope_store(const t5g_rope_store_args* g, void* stream) {
    if (!g || g->reserved || (g->X != nullptr) == (g->Xpart != nullptr)) return T5G_EINVAL;
    if (g->M <= 0 || g->D <= 0 || g->D % 2 || g->nq < 0 || g->nk < 0 || g->nv < 0 || g->nq + g->nk + g->nv <= 0 ||
        g->col0 < 0 || g->ldx < g->col0 + (g->nq + g->nk + g->nv) * g->D)
        return T5G_EINVAL;
    if (g->Xpart && (g->nsplit < 1 || g->nsplit > 8)) return T5G_EINVAL;
    if (g->nq && (!g->Qout || g->ldq < g->nq * g->D)) return T5G_EINVAL;
    if (g->nq && g->Qout == g->X && g->ldq != g->ldx) return T5G_EINVAL;
    if ((g->nk && !g->Kc) || (g->nv && !g->Vc)) return T5G_EINVAL;
    if (g->nk + g->nv > 0 && ((!g->tok_t && !g->kv_len) || g->c_hstride < g->D || g->c_bstride < 0)) return T5G_EINVAL;
    const bool rot = (g->nq && g->rope_q) || (g->nk && g->rope_k);
    if (rot && !g->rope_tab && (!g->pos || !g->inv_freq)) return T5G_EINVAL;
    RopeArgs r;
    memset(&r, 0, sizeof(r));
    r.X = (const bf16_t*)g->X;
    r.Xpart = g->Xpart;
    r.nsplit = g->Xpart ? g->nsplit : 0;
    r.ldx = g->ldx;
    r.M = g->M;
    r.D = g->D;
    r.nq = g->nq;
    r.nk = g->nk;
    r.nv = g->nv;
    r.col0 = g->col0;
    r.rope_q = g->rope_q;
    r.rope_k = g->rope_k;
    r.pos = g->pos;
    r.inv_freq = g->inv_freq;
    r.tok_row = g->tok_row;
    r.tok_t = g->tok_t;
    r.kv_len = g->kv_len;
    r.Qout = (bf16_t*)g->Qout;
    r.ldq = g->ldq;
    r.Kc = (bf16_t*)g->Kc;
    r.Vc = (bf16_t*)g->Vc;
    r.c_bstride = (long)g->c_bstride;
    r.c_hstride = (long)g->c_hstride;
    r.rope_tab = g->rope_tab;
    RC(rope_store(r, (hipStream_t)stream));
    return T5G_OK;
}

static_assert(sizeof(t5g_attn_packed_args) == 96, "t5g_attn_packed_args layout");

extern "C" int t5g_attention_packed(const t5g_attn_packed_args* g, void* stream) {
    if (!g || g->reserved || !g->q || !g->k_cache || !g->v_cache || !g->kv_len || !g->out) return T5G_EINVAL;
    if (g->Mq <= 0 || g->n_kv_heads <= 0 || g->n_heads <= 0 || g->n_heads % g->n_kv_heads || g->head_dim <= 0 ||
        g->cap <= 0 || g->window < 0 || g->softcap < 0.f)
        return T5G_EINVAL;
    const int G = g->n_heads / g->n_kv_heads;
    // an unbuilt geometry is reported as such, whatever its score footprint would be
    if (!((g->head_dim == 256 && (G == 1 || G == 2)) || (G == 2 && (g->head_dim == 64 || g->head_dim == 128))))
        return T5G_EUNSUPPORTED;
    if (g->cap > SDPA_KV_BLOCK * SDPA_MAX_BLOCKS || (size_t)G * g->cap * sizeof(float) > 96 * 1024) return T5G_EINVAL;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = (const bf16_t*)g->q;
    a.ldq = g->n_heads * g->head_dim;
    a.Mq = g->Mq;
    a.q_row = g->q_row;
    a.q_pos = g->q_pos;
    a.K = (const bf16_t*)g->k_cache;
    a.V = (const bf16_t*)g->v_cache;
    a.kv_hstride = (long)g->cap * g->head_dim;
    a.kv_bstride = a.kv_hstride * g->n_kv_heads;
    a.kv_len = g->kv_len;
    a.Hkv = g->n_kv_heads;
    a.D = g->head_dim;
    a.G = G;
    a.causal = g->causal;
    a.window = g->window;
    a.scale = g->scale;
    a.softcap = g->softcap;
    a.eager = g->softcap > 0.f;   // as attn_packed (engine.hip)
    a.nsplit = 1;
    a.chunk = g->cap;
    a.O = (bf16_t*)g->out;
    a.ldo = a.ldq;
    RC(attention(a, (hipStream_t)stream));
    return T5G_OK;
}

static_assert(sizeof(t5g_gemv_args) == 152, "t5g_gemv_args layout");

static int gemv_from_abi(const t5g_gemv_args* g, const void* W, DecGemmArgs* out) {
    if (!g || !W || !g->Y || g->M <= 0 || g->N <= 0 || g->K <= 0 || g->K % 32) return T5G_EINVAL;
    if (g->pro != 0 || g->layout < 0 || g->layout > 1) return T5G_EUNSUPPORTED;   // prologue variants were removed
    DecGemmArgs a = dec_args(g->M, W, g->N, g->K, g->Y, g->ldy, g->nw);
    a.X = (const bf16_t*)g->X;
    a.ldx = g->ldx;
    a.bias = (const bf16_t*)g->bias;
    a.un = g->un;
    a.max_grid = g->max_grid;
    a.splits = g->splits > 1 ? g->splits : 1;
    a.layout_rx = g->layout == 1;
    *out = a;
    return T5G_OK;
}

extern "C" int t5g_gemv(const t5g_gemv_args* g, void* stream) {
    DecGemmArgs a;
    int rc = gemv_from_abi(g, g ? g->W : nullptr, &a);
    if (rc) return rc;
    RC(gemv_dec(a, g->epi, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_gemv_fp8(const t5g_gemv_args* g, const float* scale, void* stream) {
    DecGemmArgs a;
    int rc = gemv_from_abi(g, g ? g->W : nullptr, &a);
    if (rc) return rc;
    if (!scale) return T5G_EINVAL;
    RC(gemv_rx_p8(a, scale, g->epi, (hipStream_t)stream));   // -1 (layout 0, an unbuilt shape): as t5g_gemv
    return T5G_OK;
}

extern "C" int t5g_time_gemv(const t5g_gemv_args* g, const void* const* Wp_list, int32_t n_w, int32_t iters,
                             void* stream, float* avg_us) {
    if (!g || !Wp_list || n_w <= 0 || iters <= 0 || !avg_us) return T5G_EINVAL;
    std::vector<DecGemmArgs> as((size_t)n_w);
    for (int i = 0; i < n_w; ++i) {
        int rc = gemv_from_abi(g, Wp_list[i], &as[i]);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    auto launch = [&](int i) -> int {
        RC(gemv_dec(as[i % n_w], g->epi, st));
        return T5G_OK;
    };
    if (const int rc = launch(0)) return rc;   // warm
    return time_loop(st, iters, launch, avg_us);
}

extern "C" int t5g_exact_linear(const void* X, int32_t ldx, int32_t M, const void* Wp, int32_t N, int32_t K,
                                int32_t kb32, const void* bias, const void* gelu_lut, void* Y, int32_t ldy, int32_t epi,
                                void* stream) {
    if (!X || !Wp || !Y || M <= 0 || N <= 0 || K <= 0 || K % 32 || kb32 < 0) return T5G_EINVAL;
    ExactLinArgs a;
    memset(&a, 0, sizeof(a));
    a.X = (const bf16_t*)X;
    a.ldx = ldx;
    a.M = M;
    a.W = (const bf16_t*)Wp;
    a.N = N;
    a.NG = ng_pad(N);
    a.KB = K / 32;
    a.bias = (const bf16_t*)bias;
    a.Y = Y;
    a.ldy = ldy;
    a.kb_fixed = kb32;
    a.gelu_lut = (const uint16_t*)gelu_lut;
    RC(exact_linear(a, epi, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_pack_e16(const void* p16, void* e16, int64_t bytes, void* stream) {
    RC(pack_e16((const bf16_t*)p16, (bf16_t*)e16, (long)bytes, (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_to_x16(const void* X, int32_t ldx, int32_t M, int32_t K, void* Y16, void* stream) {
    RC(to_x16((const bf16_t*)X, ldx, M, K, (bf16_t*)Y16, (hipStream_t)stream));
    return T5G_OK;
}

// hipEvent-timed xmm launches on E16 weights W16_list[i % n_w] (rotate past the Infinity
// Cache so every launch streams from HBM, as inside a decode step); epi | 0x1000: also the
// X16 output (Y16 = Y) instead of row-major
extern "C" int t5g_time_xmm(const void* X16, int32_t M, const void* const* W16_list, int32_t n_w, int32_t N,
                            int32_t K, int32_t epi, const void* bias, void* Y, int32_t ldy, int32_t iters,
                            void* stream, float* avg_us) {
    if (!X16 || !W16_list || n_w <= 0 || !Y || iters <= 0 || !avg_us || K % 32) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    XmmArgs a;
    memset(&a, 0, sizeof(a));
    a.X16 = (const bf16_t*)X16;
    a.M = M;
    a.N = N;
    a.NG = ng_pad(N);
    a.KB = K / 32;
    a.bias = (const bf16_t*)bias;
    if (epi & 0x1000) a.Y16 = (bf16_t*)Y;
    else a.Y = Y;
    a.ldy = ldy;
    a.timing_var = (epi & 0x4000) ? 1 : ((epi & 0x8000) ? 2 : 0);   // decode-kernel timing variants
    epi &= 0xff;
    auto launch = [&](int i) -> int {
        a.W = (const bf16_t*)W16_list[i % n_w];
        RC(xmm(a, epi, st));
        return T5G_OK;
    };
    if (const int rc = launch(0)) return rc;   // warm
    return time_loop(st, iters, launch, avg_us);
}

// The same Linear on the f32-MFMA kernels (xmm.hip): X converted to X16 and the packed W
// to E16 in temporaries (test / probe entry point; the engine keeps both resident)
extern "C" int t5g_xmm_linear(const void* X, int32_t ldx, int32_t M, const void* Wp, int32_t N, int32_t K,
                              int32_t kb32, const void* bias, const void* gelu_lut, void* Y, int32_t ldy, int32_t epi,
                              void* stream) {
    if (!X || !Wp || !Y || M <= 0 || N <= 0 || K <= 0 || K % 32 || kb32 < 0) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long wbytes = (long)ng_pad(N) * 16 * K * 2;
    const long xbytes = (long)((M + 15) / 16) * 16 * K * 2;
    bf16_t *w16 = nullptr, *x16 = nullptr;
    HIPCHK(hipMallocAsync((void**)&w16, (size_t)wbytes, st));
    HIPCHK(hipMallocAsync((void**)&x16, (size_t)xbytes, st));
    int rc = pack_e16((const bf16_t*)Wp, w16, wbytes, st);
    if (!rc) rc = to_x16((const bf16_t*)X, ldx, M, K, x16, st);
    if (!rc) {
        XmmArgs a;
        memset(&a, 0, sizeof(a));
        a.X16 = x16;
        a.M = M;
        a.W = w16;
        a.N = N;
        a.NG = ng_pad(N);
        a.KB = K / 32;
        a.bias = (const bf16_t*)bias;
        if (epi & 0x2000) {   // K parts of kb32 chunks: Y = fp32 part values [parts][M][N]
            a.part_out = (float*)Y;
            a.part_kbc = kb32;
        } else {
            a.Y = Y;
            a.ldy = ldy;
            a.kb_fixed = kb32;
        }
        a.gelu_lut = (const uint16_t*)gelu_lut;
        rc = xmm(a, epi & 0xff, st);
    }
    hipFreeAsync(w16, st);
    hipFreeAsync(x16, st);
    RC(rc);
    return T5G_OK;
}

extern "C" int t5g_eager_attention(const void* q, int32_t Mq, const int32_t* q_row, const int32_t* q_pos,
                                   const int32_t* q_len, const void* k_cache, const void* v_cache, int32_t cap,
                                   const int32_t* kv_len, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                   int32_t causal, int32_t window, float scale, float softcap,
                                   const uint16_t* tanh_lut, void* out, void* stream) {
    if (!q || !k_cache || !v_cache || !kv_len || !out || !tanh_lut || Mq <= 0 || cap <= 0 || n_kv_heads <= 0 ||
        n_heads % n_kv_heads || head_dim <= 0)
        return T5G_EINVAL;
    ExactAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = (const bf16_t*)q;
    a.ldq = n_heads * head_dim;
    a.Mq = Mq;
    a.q_row = q_row;
    a.q_pos = q_pos;
    a.q_len = q_len;
    a.K = (const bf16_t*)k_cache;
    a.V = (const bf16_t*)v_cache;
    a.kv_hstride = (long)cap * head_dim;
    a.kv_bstride = a.kv_hstride * n_kv_heads;
    a.kv_len = kv_len;
    a.Hq = n_heads;
    a.Hkv = n_kv_heads;
    a.D = head_dim;
    a.causal = causal;
    a.window = window;
    a.scale = scale;
    a.softcap = softcap;
    a.tanh_lut = tanh_lut;
    a.O = (bf16_t*)out;
    a.ldo = a.ldq;
    hipStream_t st = (hipStream_t)stream;
    float* sb = nullptr;
    HIPCHK(hipMallocAsync((void**)&sb, (size_t)Mq * n_heads * cap * 4, st));
    const int rc = eager_attention(a, sb, cap, st);
    hipFreeAsync(sb, st);
    if (rc == -3) return T5G_EUNSUPPORTED;
    RC(rc);
    return T5G_OK;
}

extern "C" int t5g_exact_attention(const void* q, int32_t Mq, const int32_t* q_row, const int32_t* q_pos,
                                   const int32_t* q_len, const void* k_cache, const void* v_cache, int32_t cap,
                                   const int32_t* kv_len, int32_t n_heads, int32_t n_kv_heads, int32_t head_dim,
                                   int32_t causal, int32_t window, float scale, int32_t threads, void* out,
                                   void* stream) {
    if (!q || !k_cache || !v_cache || !kv_len || !out || Mq <= 0 || cap <= 0 || n_kv_heads <= 0 ||
        n_heads % n_kv_heads || head_dim <= 0 || threads <= 0)
        return T5G_EINVAL;
    ExactAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = (const bf16_t*)q;
    a.ldq = n_heads * head_dim;
    a.Mq = Mq;
    a.q_row = q_row;
    a.q_pos = q_pos;
    a.q_len = q_len;
    a.K = (const bf16_t*)k_cache;
    a.V = (const bf16_t*)v_cache;
    a.kv_hstride = (long)cap * head_dim;
    a.kv_bstride = a.kv_hstride * n_kv_heads;
    a.kv_len = kv_len;
    a.Hq = n_heads;
    a.Hkv = n_kv_heads;
    a.D = head_dim;
    a.causal = causal;
    a.window = window;
    a.scale = scale;
    a.threads = threads;
    a.O = (bf16_t*)out;
    a.ldo = a.ldq;
    if (!q_pos && !q_len) {   // one query per row at its last key: the engine's decode launches (xattn.hip)
        hipStream_t st = (hipStream_t)stream;
        const int G = n_heads / n_kv_heads, nsplit = (cap + 63) / 64;
        float *sb = nullptr, *mb = nullptr;
        HIPCHK(hipMallocAsync((void**)&sb, (size_t)Mq * n_heads * cap * 4, st));
        HIPCHK(hipMallocAsync((void**)&mb, (size_t)Mq * n_kv_heads * nsplit * G * 4, st));
        const int rc = exact_attention_decode(a, sb, mb, cap, st);
        hipFreeAsync(sb, st);
        hipFreeAsync(mb, st);
        RC(rc);
        return T5G_OK;
    }
    RC(exact_attention(a, (hipStream_t)stream));
    return T5G_OK;
}

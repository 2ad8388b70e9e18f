// Engine: owns the HBM arena (KV caches, activations, sampler state) and runs the
// T5Gemma-TTS generate() phases as sequences of the gfx950 kernels; the decode
// iteration (sampler + 26-layer single-token step + predict head) is captured
// once into a hipGraph and replayed, with all per-step scalars (lengths,
// positions, tokens) living in device memory so the graph is static.
//
// Call-stack correspondence (reference hf_export/modeling_t5gemma_voice.py):
//   t5g_encode   -> :596-615 encoder + :198-230 cross K/V (computed once per call)
//   t5g_prefill  -> :630-694 BOS+prompt decoder pass, :693 last hidden, :789 head
//   t5g_decode   -> :788-848 loop body (sample_helper, embedding, decoder step)
//
// The engine's state is engine_state.h; the timing hooks (t5g_time_*) and the stand-alone op
// wrappers for tests and probes are engine_hooks.hip.
#include "engine_state.h"
#include "fp8.h"

constexpr int GRAPH_STEPS = 8;   // decode iterations per multi-step graph

// words of e->fsync: the timeout line, the fused.hip sets, the xlayer.hip sets
static size_t fsync_words(const t5g_config& c) {
    return FM_LINE + (size_t)(FM_SET_WORDS + XL_SET_WORDS) * c.n_dec_layers;
}
static unsigned* xlayer_set(t5g_engine* e, int l) {
    return e->fsync + FM_LINE + (size_t)FM_SET_WORDS * e->c.n_dec_layers + (size_t)XL_SET_WORDS * l;
}

template <typename T>
static int alloc(t5g_engine* e, T** p, int64_t n) {
    void* ptr = nullptr;
    int64_t bytes = ((n * (int64_t)sizeof(T)) + 255) / 256 * 256;
    if (hipMalloc(&ptr, (size_t)bytes) != hipSuccess) return T5G_ENOMEM;
    hipMemset(ptr, 0, (size_t)bytes);
    e->allocs.push_back(ptr);
    e->bytes += bytes;
    *p = (T*)ptr;
    return 0;
}

extern "C" int64_t t5g_packed_bytes(int32_t N, int32_t K) {
    if (K % 32) return -1;
    return (int64_t)ng_pad(N) * 16 * K * 2;
}

extern "C" int t5g_pack_weight(const void* src, int32_t N, int32_t K, int64_t ld, void* dst, void* stream) {
    if (!src || !dst || N <= 0 || K <= 0 || K % 32) return T5G_EINVAL;
    RC(pack_p16((const bf16_t*)src, N, K, ld, (bf16_t*)dst, ng_pad(N), (hipStream_t)stream));
    return T5G_OK;
}

static void drop_graphs(t5g_engine* e) {
    if (e->gexec) hipGraphExecDestroy(e->gexec);
    if (e->gexec_n) hipGraphExecDestroy(e->gexec_n);
    if (e->graph) hipGraphDestroy(e->graph);
    if (e->graph_n) hipGraphDestroy(e->graph_n);
    if (e->gexec_fwd) hipGraphExecDestroy(e->gexec_fwd);
    if (e->graph_fwd) hipGraphDestroy(e->graph_fwd);
    e->gexec = e->gexec_n = e->gexec_fwd = nullptr;
    e->graph = e->graph_n = e->graph_fwd = nullptr;
}

// The launches body(stream) issues, captured on the engine's capture stream and instantiated.
// On failure *graph / *exec are untouched and nothing is left behind; what happens to the
// engine's other graphs is the caller's business.
template <typename F>
static int capture(t5g_engine* e, F body, hipGraph_t* graph, hipGraphExec_t* exec) {
    if (!e->cap_stream) HIPCHK(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = body(e->cap_stream);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(e->cap_stream, &g);
    if (rc || ec != hipSuccess) {
        if (g) hipGraphDestroy(g);
        return rc ? rc : T5G_EHIP;
    }
    hipGraphExec_t x = nullptr;
    if (hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess) {
        hipGraphDestroy(g);
        return T5G_EHIP;
    }
    *graph = g;
    *exec = x;
    return T5G_OK;
}

extern "C" int t5g_engine_destroy(t5g_engine* e) {
    if (!e) return T5G_OK;
    drop_graphs(e);
    if (e->cap_stream) hipStreamDestroy(e->cap_stream);
    for (void* p : e->allocs) hipFree(p);
    if (e->trig_exc) hipFree(e->trig_exc);
    delete e;
    return T5G_OK;
}

extern "C" int64_t t5g_engine_workspace_bytes(const t5g_engine* e) { return e ? e->bytes : -1; }

extern "C" int t5g_engine_create(const t5g_config* cfg, const t5g_weights* w, t5g_engine** out) {
    if (!cfg || !w || !out) return T5G_EINVAL;
    const t5g_config& c = *cfg;
    if (c.hidden % 32 || c.intermediate % 32 || c.n_enc_layers > T5G_MAX_LAYERS ||
        c.n_dec_layers > T5G_MAX_LAYERS || c.max_batch <= 0 || c.max_text <= 0 || c.max_audio <= 0 ||
        c.n_heads % c.n_kv_heads || c.max_audio > SDPA_KV_BLOCK * SDPA_MAX_BLOCKS || c.max_text > 4096)
        return T5G_EINVAL;
    t5g_engine* e = new t5g_engine();
    e->c = c;
    e->w = *w;
    e->enc.assign(w->enc_layers, w->enc_layers + c.n_enc_layers);
    e->dec.assign(w->dec_layers, w->dec_layers + c.n_dec_layers);
    e->q_dim = c.n_heads * c.head_dim;
    e->kv_dim = c.n_kv_heads * c.head_dim;
    e->qkv_dim = e->q_dim + 2 * e->kv_dim;
    e->V = c.n_audio_tokens;
    e->Vpad = ng_pad(e->V) * 16;
    const int B = c.max_batch, d = c.hidden, f = c.intermediate, D = c.head_dim, Hkv = c.n_kv_heads;
    e->max_tok = B * (c.max_text > c.max_audio ? c.max_text : c.max_audio);
    const int64_t T = e->max_tok;
    int rc = 0;
    auto widest = [&](int64_t a, int64_t b) { return a > b ? a : b; };
    rc |= alloc(e, &e->h, T * d);
    rc |= alloc(e, &e->xn, T * d);
    rc |= alloc(e, &e->qkv, T * widest(e->qkv_dim, 2 * e->kv_dim));
    rc |= alloc(e, &e->q, T * e->q_dim);
    rc |= alloc(e, &e->att, T * e->q_dim);
    rc |= alloc(e, &e->act, T * f);
    rc |= alloc(e, &e->tmp, T * widest(widest(d, e->qkv_dim), 2 * e->kv_dim));
    rc |= alloc(e, &e->mem, (int64_t)B * c.max_text * d);
    // split-K slabs: decode uses up to 8 splits of [B][max(d, qkv)]
    e->part_elems = (int64_t)8 * B * widest(widest(d, e->qkv_dim), 2 * e->kv_dim);
    rc |= alloc(e, &e->part, e->part_elems);
    const int G = c.n_heads / c.n_kv_heads;
    const int nsplit_dec = (c.max_audio + 63) / 64, nsplit_x = (c.max_text + 63) / 64;
    const int nsplit_max = nsplit_dec > nsplit_x ? nsplit_dec : nsplit_x;
    const int cap_max = c.max_audio > c.max_text ? c.max_audio : c.max_text;
    rc |= alloc(e, &e->asbuf, (int64_t)B * c.n_heads * cap_max);
    rc |= alloc(e, &e->ambuf, (int64_t)B * Hkv * nsplit_max * G);
    rc |= alloc(e, &e->afpart, (int64_t)B * Hkv * nsplit_max * G * D);
    rc |= alloc(e, &e->afstat, (int64_t)B * Hkv * nsplit_max * G * 2);
    rc |= alloc(e, &e->aftick, (int64_t)B * Hkv);
    const int64_t enc_cache = (int64_t)B * Hkv * c.max_text * D;
    rc |= alloc(e, &e->enc_k, enc_cache);
    rc |= alloc(e, &e->enc_v, enc_cache);
    const int64_t self_cache = (int64_t)B * Hkv * c.max_audio * D;
    e->ck.resize(c.n_dec_layers);
    e->cv.resize(c.n_dec_layers);
    e->sk.resize(c.n_dec_layers);
    e->sv.resize(c.n_dec_layers);
    for (int l = 0; l < c.n_dec_layers; ++l) {
        rc |= alloc(e, &e->ck[l], enc_cache);
        rc |= alloc(e, &e->cv[l], enc_cache);
        rc |= alloc(e, &e->sk[l], self_cache);
        rc |= alloc(e, &e->sv[l], self_cache);
    }
    rc |= alloc(e, &e->enc_len, B);
    rc |= alloc(e, &e->dh, (int64_t)B * d);
    rc |= alloc(e, &e->dxn, (int64_t)B * d);
    rc |= alloc(e, &e->dq, (int64_t)B * e->q_dim);
    rc |= alloc(e, &e->datt, (int64_t)B * e->q_dim);
    rc |= alloc(e, &e->dact, (int64_t)B * f);
    rc |= alloc(e, &e->dhh, (int64_t)B * d);
    e->logits_ld = e->Vpad;
    rc |= alloc(e, &e->logits, (int64_t)B * e->logits_ld);
    rc |= alloc(e, &e->rows, B);
    rc |= alloc(e, &e->state, B);
    rc |= alloc(e, &e->topk_list, 4096);
    rc |= alloc(e, &e->silence, 4096);
    rc |= alloc(e, &e->out_tokens, (int64_t)B * (c.max_gen > 0 ? c.max_gen : 1));
    rc |= alloc(e, &e->kv_len, B);
    rc |= alloc(e, &e->next_pos, B);
    rc |= alloc(e, &e->next_token, B);
    rc |= alloc(e, &e->flags, B);
    rc |= alloc(e, &e->last_rows, B);
    rc |= alloc(e, &e->rope_tab, (int64_t)B * D);
    rc |= alloc(e, &e->fs_val, (int64_t)B * FS_NB * FS_CAP);
    rc |= alloc(e, &e->fs_idx, (int64_t)B * FS_NB * FS_CAP);
    rc |= alloc(e, &e->fs_cnt, (int64_t)B * FS_NB);
    rc |= alloc(e, &e->fs_amv, (int64_t)B * FS_NB);
    rc |= alloc(e, &e->fs_ami, (int64_t)B * FS_NB);
    rc |= alloc(e, &e->fs_ticket, B);
    rc |= alloc(e, &e->fs_slow, B);
    rc |= alloc(e, &e->part2, (int64_t)2 * B * e->q_dim + (int64_t)4 * B * d + (int64_t)8 * B * d + (int64_t)4 * B * d);
    rc |= alloc(e, &e->datt2, (int64_t)B * e->q_dim);
    rc |= alloc(e, &e->fsync, (int64_t)fsync_words(c));
    if (rc) {
        t5g_engine_destroy(e);
        return T5G_ENOMEM;
    }
    *out = e;
    return T5G_OK;
}

// ---------------------------------------------------------------------------
// The engine's encoder / prefill GEMMs run the LDS-staged kernel (gemm_pfl_kernel). Round 3
// had moved them to the register ring because the last token tile's sums varied from run
// to run: a wave could reach the ring's barrier with its own ds_reads of the slot still in
// flight while the DMA refilled it; the barrier now waits for lgkmcnt(0) too (gemm.hip
// wait_vm_barrier; tests/test_gpu_prefill_lds.py, tools/diag_det_logits.py).
int gemm(const bf16_t* X, int ldx, int M, const void* W, int N, int K, int splits, const void* bias, void* Y, int ldy,
         int epi, hipStream_t st, bool prefill, bool pf_reg) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.prefill = prefill ? (pf_reg ? 2 : 1) : 0;
    a.X = X;
    a.ldx = ldx;
    a.M = M;
    a.W = (const bf16_t*)W;
    a.N = N;
    a.NG = ng_pad(N);
    a.KB = K / 32;
    a.splits = splits;
    a.bias = (const bf16_t*)bias;
    a.Y = Y;
    a.ldy = ldy;
    return gemm_p16(a, epi, st);
}

NormArgs norm_args(int M, int d, float eps) {
    NormArgs n;
    memset(&n, 0, sizeof(n));
    n.M = M;
    n.d = d;
    n.eps = eps;
    return n;
}

// Self-attention block input is xn (normed) -> result residual update.
// Packed-token path (encoder / prefill / cross prefill) -------------------------------
static int attn_packed(t5g_engine* e, int ntok, const bf16_t* q, const int* tok_row, const int* tok_t,
                       const bf16_t* K, const bf16_t* Vc, int Lmax, const int* kv_len, int causal, int window,
                       bf16_t* out, hipStream_t st) {
    const t5g_config& c = e->c;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = q;
    a.ldq = e->q_dim;
    a.Mq = ntok;
    a.q_row = tok_row;
    a.q_pos = tok_t;
    a.K = K;
    a.V = Vc;
    a.kv_hstride = (long)Lmax * c.head_dim;
    a.kv_bstride = a.kv_hstride * c.n_kv_heads;
    a.kv_len = kv_len;
    a.Hkv = c.n_kv_heads;
    a.D = c.head_dim;
    a.G = c.n_heads / c.n_kv_heads;
    a.causal = causal;
    a.window = window;
    a.scale = c.attn_scale;
    a.softcap = c.softcap;
    a.eager = c.softcap > 0.f;
    a.nsplit = 1;
    a.chunk = Lmax;
    a.O = out;
    a.ldo = e->q_dim;
    return attention(a, st);
}

// ---------------------------------------------------------------------------
// Parity mode: the same phases on the exact-order kernels (exact.hip, norm.hip EXACT),
// unfused, with every tensor rounded where the reference's bf16 tensor ops round it.
static const uint16_t* ksplit_tab(const t5g_engine* e, int N, int K) {
    if (!e->ksplit_dev) return nullptr;
    for (int i = 0; i < REF_KSPLIT_NSHAPES; ++i)
        if (ref_ksplit_shapes[i].N == N && ref_ksplit_shapes[i].K == K) return e->ksplit_dev + (long)i * REF_KSPLIT_MAX_M;
    return nullptr;   // shapes never split by the reference host (K <= 256 in the probes)
}

// Exact Linear on the f32 MFMA: X16 operand, E16 weights; Y row-major and / or Y16.
// nref_a / nref_b: the reference Linear's output width for packed columns < / >= nsplit_col
// (q | k,v share one packed matrix here but are separate F.linear calls there)
int xlin16(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, const void* bias, void* Y,
           int ldy, bf16_t* Y16, int epi, const int* tok_row, const int* row_len, int nref_a, int nref_b,
           int nsplit_col, hipStream_t st) {
    XmmArgs a;
    memset(&a, 0, sizeof(a));
    a.X16 = X16;
    a.M = M;
    a.W = W16;
    a.N = N;
    a.NG = ng_pad(N);
    a.KB = K / 32;
    a.bias = (const bf16_t*)bias;
    a.Y = Y;
    a.ldy = ldy;
    a.Y16 = Y16;
    a.tok_row = tok_row;
    a.row_len = row_len;
    a.kb_a = ksplit_tab(e, nref_a, K);
    a.kb_b = nref_b ? ksplit_tab(e, nref_b, K) : nullptr;
    a.nsplit_col = nsplit_col;
    a.kb_len = REF_KSPLIT_MAX_M;
    a.gelu_lut = e->gelu_lut_dev;
    return xmm(a, epi, st);
}

// The reference's K part (chunks) of Linear (N, K) called with M rows; KB when not split
static int ksplit_host(int N, int K, int M) {
    for (int i = 0; i < REF_KSPLIT_NSHAPES; ++i)
        if (ref_ksplit_shapes[i].N == N && ref_ksplit_shapes[i].K == K && M >= 1 && M <= ref_ksplit_max_m[i]) {
            const int v = ref_ksplit_kb32[i][M - 1];
            return v > 0 ? v : K / 32;
        }
    return K / 32;
}

// Decode rows (each a reference call of M = 1): when the reference splits K at M = 1, one
// workgroup per (group, part) writes the parts' fp32 values to e->dpart and the number of
// parts is returned in *nparts (the consumer norm folds them); otherwise a plain bf16 Linear
// into Y (*nparts = 0).
int xlin16_dec_parts(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, void* Y, int ldy,
                     const int* tok_row, int* nparts, hipStream_t st) {
    const int kbc = ksplit_host(N, K, 1), KB = K / 32;
    *nparts = 0;
    if (kbc >= KB || M > 32 || (KB + kbc - 1) / kbc > 4 || N > e->c.hidden)
        return xlin16(e, X16, M, W16, N, K, nullptr, Y, ldy, nullptr, EPI_BF16, tok_row, nullptr, N, 0, 0, st);
    XmmArgs a;
    memset(&a, 0, sizeof(a));
    a.X16 = X16;
    a.M = M;
    a.W = W16;
    a.N = N;
    a.NG = ng_pad(N);
    a.KB = KB;
    a.part_out = e->dpart;
    a.part_kbc = kbc;
    RC(xmm(a, EPI_F32, st));
    *nparts = (KB + kbc - 1) / kbc;
    return T5G_OK;
}

// fr (decode only, exact_attention_decode_supported): RoPE fused into the scores launch --
// Q un-rotated, rotated with the step's table; with kv_new also the new key / value appended
struct XattnFuse {
    const float* rope_tab = nullptr;
    const bf16_t* kv_new = nullptr;
    int ld_new = 0, k_col0 = 0, v_col0 = 0;
    int ldq = 0;   // row stride of Q when it is not q_dim (the q | k | v buffer)
    int span_max = 0;   // host bound on every row's keys (0: cap)
};
static int xattn(t5g_engine* e, const bf16_t* Q, int Mq, const int* q_row, const int* q_pos, const int* q_len,
                 const bf16_t* K, const bf16_t* Vc, int cap, const int* kv_len, int causal, int window, bf16_t* O,
                 bf16_t* O16, hipStream_t st, const XattnFuse& fr = XattnFuse()) {
    const t5g_config& c = e->c;
    ExactAttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = Q;
    a.ldq = fr.ldq ? fr.ldq : e->q_dim;
    a.Mq = Mq;
    a.q_row = q_row;
    a.q_pos = q_pos;
    a.q_len = q_len;
    a.K = K;
    a.V = Vc;
    a.kv_hstride = (long)cap * c.head_dim;
    a.kv_bstride = a.kv_hstride * c.n_kv_heads;
    a.kv_len = kv_len;
    a.Hq = c.n_heads;
    a.Hkv = c.n_kv_heads;
    a.D = c.head_dim;
    a.causal = causal;
    a.window = window;
    a.scale = c.attn_scale;
    a.threads = e->exact_threads;
    a.O = O;
    a.ldo = e->q_dim;
    a.O16 = O16;
    a.rope_tab = fr.rope_tab;
    a.kv_new = fr.kv_new;
    a.ld_new = fr.ld_new;
    a.k_col0 = fr.k_col0;
    a.v_col0 = fr.v_col0;
    a.span_max = fr.span_max;
    if (c.softcap > 0.f) {
        // eager attention (eager.hip): decode rows on the engine's scores scratch, packed
        // (prefill / encoder) calls on a stream-ordered one (not inside a captured graph)
        a.softcap = c.softcap;
        a.tanh_lut = e->tanh_lut_dev;
        if (!q_pos && !q_len) return eager_attention(a, e->asbuf, cap, st);
        float* sb = nullptr;
        if (hipMallocAsync((void**)&sb, (size_t)Mq * c.n_heads * cap * sizeof(float), st) != hipSuccess) return -2;
        const int rc = eager_attention(a, sb, cap, st);
        hipFreeAsync(sb, st);
        return rc;
    }
    // decode rows (one query each): the scores + P.V launches of xattn.hip
    if (!q_pos && !q_len) {
        const int rc = exact_attention_decode(a, e->asbuf, e->ambuf, cap, st);
        if (rc != -3 || fr.rope_tab) return rc;   // -3: a head shape the decode kernels are not built for
    }
    if (fr.rope_tab) return -1;
    return exact_attention(a, st);
}

static NormArgs xnorm_args(int M, int d, float eps) {
    NormArgs n;
    memset(&n, 0, sizeof(n));
    n.M = M;
    n.d = d;
    n.eps = eps;
    n.exact = 1;
    return n;
}

static RopeArgs xrope_args(const t5g_engine* e, int M, int D, const float* pos, const float* inv_freq,
                           const int* tok_row, const int* tok_t, const int* kv_len) {
    RopeArgs r;
    memset(&r, 0, sizeof(r));
    r.trig_exc = e->trig_exc;
    r.n_trig_exc = e->n_trig_exc;
    r.M = M;
    r.D = D;
    r.pos = pos;
    r.inv_freq = inv_freq;
    r.tok_row = tok_row;
    r.tok_t = tok_t;
    r.kv_len = kv_len;
    r.exact_trig = 1;
    return r;
}

static int encode_exact(t5g_engine* e, int ntok, const int32_t* ids, const int32_t* tok_row, const int32_t* tok_t,
                        const float* pos, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate, D = c.head_dim;
    const int* rl = e->enc_len;   // the reference encodes one utterance: M = its text length
    for (int l = 0; l < c.n_enc_layers; ++l) {
        const t5g_layer_weights& L = e->enc[l];
        const t5g_engine::XLayer& X = e->enc_x[l];
        NormArgs n = xnorm_args(ntok, d, c.rms_eps);
        if (l == 0) {
            n.ids = ids;
            n.table = (const bf16_t*)e->w.enc_embed;
            n.n_table = c.text_vocab;
            n.scale = c.normalizer;
        } else {
            n.delta = e->tmp;
            n.post_w = (const bf16_t*)e->enc[l - 1].norms[5];
            n.resid = e->h;
        }
        n.pre_w = (const bf16_t*)L.norms[0];
        n.resid_out = e->h;
        n.normed_out = e->xn;
        n.normed_x16 = e->xn16;
        RC(resid_norm(n, st));
        RC(xlin16(e, e->xn16, ntok, X.qkv, e->qkv_dim, d, nullptr, e->qkv, e->qkv_dim, nullptr, EPI_BF16, tok_row, rl,
                  e->q_dim, e->kv_dim, e->q_dim, st));
        RopeArgs r = xrope_args(e, ntok, D, pos, e->w.inv_freq, tok_row, tok_t, nullptr);
        r.X = e->qkv;
        r.ldx = e->qkv_dim;
        r.nq = c.n_heads;
        r.nk = r.nv = c.n_kv_heads;
        r.rope_q = r.rope_k = 1;
        r.Qout = e->q;
        r.ldq = e->q_dim;
        r.Kc = e->enc_k;
        r.Vc = e->enc_v;
        r.c_hstride = (long)c.max_text * D;
        r.c_bstride = r.c_hstride * c.n_kv_heads;
        RC(rope_store(r, st));
        RC(xattn(e, e->q, ntok, tok_row, tok_t, rl, e->enc_k, e->enc_v, c.max_text, rl, 0,
                 c.enc_sliding[l] ? c.sliding_window : 0, e->att, e->att16, st));
        RC(xlin16(e, e->att16, ntok, X.o, d, e->q_dim, nullptr, e->tmp, d, nullptr, EPI_BF16, tok_row, rl, d, 0, 0,
                  st));
        n = xnorm_args(ntok, d, c.rms_eps);
        n.delta = e->tmp;
        n.post_w = (const bf16_t*)L.norms[1];
        n.resid = e->h;
        n.pre_w = (const bf16_t*)L.norms[4];
        n.resid_out = e->h;
        n.normed_out = e->xn;
        n.normed_x16 = e->xn16;
        RC(resid_norm(n, st));
        RC(xlin16(e, e->xn16, ntok, X.gate_up, 2 * f, d, nullptr, nullptr, f, e->act16, EPI_GEGLU, tok_row, rl, f, 0,
                  0, st));
        RC(xlin16(e, e->act16, ntok, X.down, d, f, nullptr, e->tmp, d, nullptr, EPI_BF16, tok_row, rl, d, 0, 0, st));
    }
    NormArgs n = xnorm_args(ntok, d, c.rms_eps);
    n.delta = e->tmp;
    n.post_w = (const bf16_t*)e->enc[c.n_enc_layers - 1].norms[5];
    n.resid = e->h;
    n.pre_w = (const bf16_t*)e->w.enc_final_norm;
    n.resid_out = e->h;
    n.normed_out = e->mem;
    n.normed_x16 = e->mem16;
    RC(resid_norm(n, st));
    for (int l = 0; l < c.n_dec_layers; ++l) {
        RC(xlin16(e, e->mem16, ntok, e->dec_x[l].cross_kv, 2 * e->kv_dim, d, nullptr, e->qkv, 2 * e->kv_dim, nullptr,
                  EPI_BF16, tok_row, rl, e->kv_dim, e->kv_dim, e->kv_dim, st));
        RopeArgs r = xrope_args(e, ntok, D, pos, e->w.inv_freq, tok_row, tok_t, nullptr);
        r.X = e->qkv;
        r.ldx = 2 * e->kv_dim;
        r.nk = r.nv = c.n_kv_heads;
        r.rope_k = 1;
        r.Kc = e->ck[l];
        r.Vc = e->cv[l];
        r.c_hstride = (long)c.max_text * D;
        r.c_bstride = r.c_hstride * c.n_kv_heads;
        RC(rope_store(r, st));
    }
    return T5G_OK;
}

// Parity decode rows through xlayer.hip (the layer after the self attention as one launch):
// the 2b-2b shapes, M <= 8 rows, <= 64 text keys per row (the call's hint), no softcap, and
// the reference splitting none of the layer's M = 1 Linears but the down projection, in two
// K parts of 144 chunks (ref_ksplit.h) -- the arithmetic the launch is built for
bool xlayer_usable(const t5g_engine* e, int M) {
    const t5g_config& c = e->c;
    if (!e->fused_mlp || M < 1 || M > 8 || c.softcap > 0.f || c.n_dec_layers < 2) return false;
    if (c.hidden != 2304 || c.intermediate != 9216 || e->q_dim != 2048 || e->kv_dim != 1024 || c.head_dim != 256 ||
        c.n_heads != 8 || c.n_kv_heads != 4 || e->qkv_dim != 4096)
        return false;
    if ((e->text_max > 0 ? e->text_max : c.max_text) > 64) return false;
    auto whole = [](int N, int K) { return ksplit_host(N, K, 1) >= K / 32; };
    return whole(2304, 2048) && whole(2048, 2304) && whole(9216, 2304) && whole(1024, 2304) &&
           ksplit_host(2304, 9216, 1) == 144;
}

XLayerArgs xlayer_args(t5g_engine* e, int M, int l) {
    const t5g_config& c = e->c;
    const t5g_layer_weights& L = e->dec[l];
    const t5g_engine::XLayer& X = e->dec_x[l];
    const bool last = l == c.n_dec_layers - 1;
    XLayerArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M;
    a.Wo = X.o;
    a.Wq = X.cross_q;
    a.Wco = X.cross_o;
    a.Wgu = X.gate_up;
    a.Wd = X.down;
    a.Wqkv = last ? nullptr : e->dec_x[l + 1].qkv;
    a.n1_post = (const bf16_t*)L.norms[1];
    a.n1_pre = (const bf16_t*)L.norms[2];
    a.n2_post = (const bf16_t*)L.norms[3];
    a.n2_pre = (const bf16_t*)L.norms[4];
    a.n3_post = (const bf16_t*)L.norms[5];
    a.n3_pre = (const bf16_t*)(last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]);
    a.eps = c.rms_eps;
    a.att16_self = e->datt16;
    a.h = e->dh;
    a.xn = e->dxn;
    a.xn16 = e->dxn16;
    a.tmp = e->tmp;
    a.q = e->dq;
    a.att = e->datt;
    a.att16 = e->datt16;
    a.act16 = e->dact16;
    a.dpart = e->dpart;
    a.qkv = e->qkv;
    a.qkv_dim = e->qkv_dim;
    a.ck = e->ck[l];
    a.cv = e->cv[l];
    a.kv_hstride = (long)c.max_text * c.head_dim;
    a.kv_bstride = a.kv_hstride * c.n_kv_heads;
    a.enc_len = e->enc_len;
    a.rope_tab = e->rope_tab;
    a.scale = c.attn_scale;
    a.sync = xlayer_set(e, l);
    a.sync_next = xlayer_set(e, (l + 1) % c.n_dec_layers);
    a.timeout = e->fsync;
    return a;
}

// decode: M = B rows fed by the sampler buffers (the reference's M = 1 per call);
// prefill: M packed tokens, the reference's M = the row's token count (kv_len)
static int decoder_pass_exact(t5g_engine* e, int M, const int* ids, const int* tok_row, const int* tok_t,
                              const float* pos, bool decode, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate, D = c.head_dim;
    bf16_t* h = decode ? e->dh : e->h;
    bf16_t* xn = decode ? e->dxn : e->xn;
    bf16_t* xn16 = decode ? e->dxn16 : e->xn16;
    bf16_t* q = decode ? e->dq : e->q;
    bf16_t* att = decode ? e->datt : e->att;
    bf16_t* att16 = decode ? e->datt16 : e->att16;
    bf16_t* act16 = decode ? e->dact16 : e->act16;
    bf16_t* tmp = e->tmp;
    const int* rl = decode ? nullptr : e->kv_len;
    const int* qlen = decode ? nullptr : e->kv_len;
    auto norm = [&](const void* post_w, const void* pre_w) -> int {
        NormArgs n = xnorm_args(M, d, c.rms_eps);
        n.delta = tmp;
        n.post_w = (const bf16_t*)post_w;
        n.resid = h;
        n.pre_w = (const bf16_t*)pre_w;
        n.resid_out = h;
        n.normed_out = xn;
        n.normed_x16 = xn16;
        return resid_norm(n, st);
    };
    // decode: the rest of each layer as one xlayer.hip launch, which also runs the next
    // layer's q|k|v (bitwise equal to the per-op launches below)
    bool xl = decode && xlayer_usable(e, M) && exact_attention_decode_supported(c.n_heads / c.n_kv_heads, D);
    bool qkv_done = false;
    for (int l = 0; l < c.n_dec_layers; ++l) {
        const t5g_layer_weights& L = e->dec[l];
        const t5g_engine::XLayer& X = e->dec_x[l];
        if (l == 0) {
            NormArgs n = xnorm_args(M, d, c.rms_eps);
            n.ids = ids;
            n.table = (const bf16_t*)e->w.audio_embed;
            n.n_table = c.n_audio_tokens;
            n.scale = c.normalizer;
            n.pre_w = (const bf16_t*)L.norms[0];
            n.resid_out = h;
            n.normed_out = xn;
            n.normed_x16 = xn16;
            if (decode) {   // and the step's RoPE table (exact cos / sin), in the same launch
                n.rope_pos = pos;
                n.rope_inv_freq = e->w.inv_freq;
                n.rope_tab = e->rope_tab;
                n.rope_D = D;
                n.trig_exc = e->trig_exc;
                n.n_trig_exc = e->n_trig_exc;
            }
            RC(resid_norm(n, st));
        }
        // self attention
        if (!qkv_done)
            RC(xlin16(e, xn16, M, X.qkv, e->qkv_dim, d, nullptr, e->qkv, e->qkv_dim, nullptr, EPI_BF16, tok_row, rl,
                      e->q_dim, e->kv_dim, e->q_dim, st));
        qkv_done = false;
        // decode: RoPE of q and k and the cache append happen inside the scores launch
        const bool fuse = decode && exact_attention_decode_supported(c.n_heads / c.n_kv_heads, D);
        if (fuse) {
            XattnFuse fr;
            fr.rope_tab = e->rope_tab;
            fr.kv_new = e->qkv;
            fr.span_max = e->audio_max;   // the call's key bound (0: max_audio)
            fr.ld_new = e->qkv_dim;
            fr.k_col0 = e->q_dim;
            fr.v_col0 = e->q_dim + e->kv_dim;
            fr.ldq = e->qkv_dim;
            RC(xattn(e, e->qkv, M, tok_row, tok_t, qlen, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1,
                     c.dec_sliding[l] ? c.sliding_window : 0, att, att16, st, fr));
            if (xl) {
                const int rc = xlayer_launch(xlayer_args(e, M, l), st);
                if (rc == 0) {
                    ++e->xl_launches;
                    qkv_done = l + 1 < c.n_dec_layers;
                    continue;
                }
                if (rc != -1 || l > 0) return rc == -1 ? T5G_EINVAL : rc;   // -1 is static: all layers or none
                xl = false;
            }
        } else {
            RopeArgs r = xrope_args(e, M, D, pos, e->w.inv_freq, tok_row, tok_t, e->kv_len);
            r.rope_tab = decode ? e->rope_tab : nullptr;
            r.X = e->qkv;
            r.ldx = e->qkv_dim;
            r.nq = c.n_heads;
            r.nk = r.nv = c.n_kv_heads;
            r.rope_q = r.rope_k = 1;
            r.Qout = q;
            r.ldq = e->q_dim;
            r.Kc = e->sk[l];
            r.Vc = e->sv[l];
            r.c_hstride = (long)c.max_audio * D;
            r.c_bstride = r.c_hstride * c.n_kv_heads;
            RC(rope_store(r, st));
            RC(xattn(e, q, M, tok_row, tok_t, qlen, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1,
                     c.dec_sliding[l] ? c.sliding_window : 0, att, att16, st));
        }
        RC(xlin16(e, att16, M, X.o, d, e->q_dim, nullptr, tmp, d, nullptr, EPI_BF16, tok_row, rl, d, 0, 0, st));
        RC(norm(L.norms[1], L.norms[2]));
        // PM cross attention
        RC(xlin16(e, xn16, M, X.cross_q, e->q_dim, d, nullptr, q, e->q_dim, nullptr, EPI_BF16, tok_row, rl, e->q_dim, 0,
                  0, st));
        if (fuse) {   // q RoPE inside the scores launch
            XattnFuse fr;
            fr.rope_tab = e->rope_tab;
            fr.span_max = e->text_max;   // the call's longest text (host hint): <= 64 keys -> one launch
            RC(xattn(e, q, M, tok_row, tok_t, qlen, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, att, att16, st,
                     fr));
        } else {
            RopeArgs r = xrope_args(e, M, D, pos, e->w.inv_freq, tok_row, tok_t, e->kv_len);
            r.rope_tab = decode ? e->rope_tab : nullptr;
            r.X = q;
            r.ldx = e->q_dim;
            r.nq = c.n_heads;
            r.rope_q = 1;
            r.Qout = q;
            r.ldq = e->q_dim;
            RC(rope_store(r, st));
            XattnFuse fr;
            fr.span_max = e->text_max;   // decode rows: the call's longest text (<= 64 keys -> one launch)
            RC(xattn(e, q, M, tok_row, tok_t, qlen, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, att, att16,
                     st, fr));
        }
        RC(xlin16(e, att16, M, X.cross_o, d, e->q_dim, nullptr, tmp, d, nullptr, EPI_BF16, tok_row, rl, d, 0, 0, st));
        RC(norm(L.norms[3], L.norms[4]));
        // GeGLU MLP: act straight into the down projection's operand order
        RC(xlin16(e, xn16, M, X.gate_up, 2 * f, d, nullptr, nullptr, f, act16, EPI_GEGLU, tok_row, rl, f, 0, 0, st));
        const bool last = l == c.n_dec_layers - 1;
        if (decode) {
            int np = 0;
            RC(xlin16_dec_parts(e, act16, M, X.down, d, f, tmp, d, tok_row, &np, st));
            NormArgs n = xnorm_args(M, d, c.rms_eps);
            if (np) {
                n.part = e->dpart;
                n.nsplit = np;
                n.ldp = d;
            } else {
                n.delta = tmp;
            }
            n.post_w = (const bf16_t*)L.norms[5];
            n.resid = h;
            n.pre_w = (const bf16_t*)(last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]);
            n.resid_out = h;
            n.normed_out = xn;
            n.normed_x16 = xn16;
            RC(resid_norm(n, st));
        } else {
            RC(xlin16(e, act16, M, X.down, d, f, nullptr, tmp, d, nullptr, EPI_BF16, tok_row, rl, d, 0, 0, st));
            RC(norm(L.norms[5], last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]));
        }
    }
    return T5G_OK;
}

// xn_rows16: the final-normed rows in X16 (decode: dxn16; prefill: the gathered last rows)
static int head_exact(t5g_engine* e, const bf16_t* xn_rows16, int B, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden;
    RC(xlin16(e, xn_rows16, B, e->head1_x, d, d, e->w.head1_bias, nullptr, d, e->dhh16, EPI_BIAS_GELU, nullptr,
              nullptr, d, 0, 0, st));
    RC(xlin16(e, e->dhh16, B, e->head2_x, e->V, d, e->w.head2_bias, e->logits, e->logits_ld, nullptr, EPI_BIAS_BF16,
              nullptr, nullptr, e->V, 0, 0, st));
    return T5G_OK;
}

// E16 copies of every packed weight + the X16 activation buffers (first switch to parity mode)
static int xmm_prepare(t5g_engine* e) {
    if (e->xmm_ready) return T5G_OK;
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate;
    hipStream_t st = nullptr;
    auto copy = [&](const void* p16, int N, int K, bf16_t** out) -> int {
        const int64_t bytes = (int64_t)ng_pad(N) * 16 * K * 2;
        RC(alloc(e, out, bytes / 2));
        RC(pack_e16((const bf16_t*)p16, *out, (long)bytes, st));
        return T5G_OK;
    };
    e->enc_x.assign(c.n_enc_layers, t5g_engine::XLayer{});
    e->dec_x.assign(c.n_dec_layers, t5g_engine::XLayer{});
    for (int l = 0; l < c.n_enc_layers; ++l) {
        const t5g_layer_weights& L = e->enc[l];
        t5g_engine::XLayer& X = e->enc_x[l];
        RC(copy(L.qkv, e->qkv_dim, d, &X.qkv));
        RC(copy(L.o, d, e->q_dim, &X.o));
        RC(copy(L.gate_up, 2 * f, d, &X.gate_up));
        RC(copy(L.down, d, f, &X.down));
    }
    for (int l = 0; l < c.n_dec_layers; ++l) {
        const t5g_layer_weights& L = e->dec[l];
        t5g_engine::XLayer& X = e->dec_x[l];
        RC(copy(L.qkv, e->qkv_dim, d, &X.qkv));
        RC(copy(L.o, d, e->q_dim, &X.o));
        RC(copy(L.gate_up, 2 * f, d, &X.gate_up));
        RC(copy(L.down, d, f, &X.down));
        RC(copy(L.cross_q, e->q_dim, d, &X.cross_q));
        RC(copy(L.cross_kv, 2 * e->kv_dim, d, &X.cross_kv));
        RC(copy(L.cross_o, d, e->q_dim, &X.cross_o));
    }
    RC(copy(e->w.head1, d, d, &e->head1_x));
    RC(copy(e->w.head2, e->V, d, &e->head2_x));
    const int64_t T16 = ((int64_t)e->max_tok + 15) / 16 * 16;
    const int64_t B16 = ((int64_t)c.max_batch + 15) / 16 * 16;
    const int64_t X16T = ((int64_t)c.max_batch * c.max_text + 15) / 16 * 16;
    RC(alloc(e, &e->xn16, T16 * d));
    RC(alloc(e, &e->att16, T16 * e->q_dim));
    RC(alloc(e, &e->act16, T16 * f));
    RC(alloc(e, &e->mem16, X16T * d));
    RC(alloc(e, &e->dxn16, B16 * d));
    RC(alloc(e, &e->datt16, B16 * e->q_dim));
    RC(alloc(e, &e->dact16, B16 * f));
    RC(alloc(e, &e->dhh16, B16 * d));
    RC(alloc(e, &e->dpart, 4 * B16 * d));
    HIPCHK(hipDeviceSynchronize());
    e->xmm_ready = true;
    return T5G_OK;
}

extern "C" int t5g_engine_set_exact(t5g_engine* e, int32_t enable, const uint16_t* gelu_lut, int32_t threads) {
    if (!e) return T5G_EINVAL;
    if (!enable) {
        if (e->exact) drop_graphs(e);
        e->exact = false;
        return T5G_OK;
    }
    if (e->fp8) return T5G_EUNSUPPORTED;   // FP8 mode is fast path only (the reference has bf16 weights)
    if (threads != REF_KSPLIT_THREADS) return T5G_EUNSUPPORTED;   // the only measured K-split table
    // eager attention (softcap): restated for the measured call shape (8 query heads of 256,
    // eager.hip) once the reference host's tanh table is set (t5g_engine_set_tanh_lut)
    if (e->c.softcap > 0.f && (!e->tanh_lut_dev || e->c.head_dim != 256 || e->c.n_heads != 8))
        return T5G_EUNSUPPORTED;
    RC(xmm_prepare(e));
    if (!e->ksplit_dev) {
        RC(alloc(e, &e->ksplit_dev, (int64_t)REF_KSPLIT_NSHAPES * REF_KSPLIT_MAX_M));
        HIPCHK(hipMemcpy(e->ksplit_dev, ref_ksplit_kb32, sizeof(ref_ksplit_kb32), hipMemcpyHostToDevice));
    }
    if (gelu_lut) {
        if (!e->gelu_lut_dev) RC(alloc(e, &e->gelu_lut_dev, 65536));
        HIPCHK(hipMemcpy(e->gelu_lut_dev, gelu_lut, 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    e->exact_threads = threads;
    if (!e->exact) drop_graphs(e);
    e->exact = true;
    return T5G_OK;
}

extern "C" int t5g_engine_set_fp8_weights(t5g_engine* e, const t5g_fp8_weights* w) {
    if (!e) return T5G_EINVAL;
    if (e->exact) return T5G_EUNSUPPORTED;   // parity mode reproduces the reference's bf16 weights
    if (w) {
        const t5g_config& c = e->c;
        // the widths of the register-X GEMV sites (decode_plan): only those run on P8
        if (c.hidden != 2304 || c.intermediate != 9216 || e->q_dim != 2048) return T5G_EUNSUPPORTED;
        if (!w->dec_layers || !w->head2.p8 || !w->head2.scale) return T5G_EINVAL;
        for (int l = 0; l < c.n_dec_layers; ++l) {
            const t5g_fp8_layer& L = w->dec_layers[l];
            for (const t5g_fp8_linear* x : {&L.qkv, &L.o, &L.cross_q, &L.cross_o, &L.gate_up, &L.down})
                if (!x->p8 || !x->scale) return T5G_EINVAL;
        }
    }
    drop_graphs(e);   // captured steps hold the other format's launches
    e->fp8 = w != nullptr;
    if (!w) e->fp8_block = e->fp8_mlp = false;   // the switches belong to FP8 mode
    e->dec8.clear();
    e->head2_8 = {nullptr, nullptr};
    if (w) {
        e->dec8.assign(w->dec_layers, w->dec_layers + e->c.n_dec_layers);
        e->head2_8 = w->head2;
    }
    return T5G_OK;
}

extern "C" int t5g_engine_weight_format(t5g_engine* e, int32_t* fmt) {
    if (!e || !fmt) return T5G_EINVAL;
    *fmt = e->fp8 ? 1 : 0;
    return T5G_OK;
}

extern "C" int t5g_engine_set_fp8_block(t5g_engine* e, int32_t enable) {
    if (!e) return T5G_EINVAL;
    if (enable && !e->fp8) return T5G_EUNSUPPORTED;
    if (e->fp8_block != (enable != 0)) {
        e->fp8_block = enable != 0;
        drop_graphs(e);   // captured launches follow the flag
    }
    return T5G_OK;
}

extern "C" int t5g_engine_set_fp8_mlp(t5g_engine* e, int32_t enable) {
    if (!e) return T5G_EINVAL;
    if (enable && !e->fp8) return T5G_EUNSUPPORTED;
    if (e->fp8_mlp != (enable != 0)) {
        e->fp8_mlp = enable != 0;
        drop_graphs(e);   // captured launches follow the flag
    }
    return T5G_OK;
}

extern "C" int t5g_engine_set_tanh_lut(t5g_engine* e, const uint16_t* lut) {
    if (!e || !lut) return T5G_EINVAL;
    if (!e->tanh_lut_dev) RC(alloc(e, &e->tanh_lut_dev, 65536));
    HIPCHK(hipMemcpy(e->tanh_lut_dev, lut, 65536 * sizeof(uint16_t), hipMemcpyHostToDevice));
    return T5G_OK;
}

extern "C" int t5g_engine_set_sampler_path(t5g_engine* e, int32_t single_block) {
    if (!e) return T5G_EINVAL;
    const bool fast = single_block == 0;
    if (fast != e->fast_sampler) drop_graphs(e);   // the sampler launch is baked into the graphs
    e->fast_sampler = fast;
    return T5G_OK;
}

extern "C" int t5g_encode(t5g_engine* e, int32_t B, int32_t ntok, const int32_t* ids, const int32_t* tok_row,
                          const int32_t* tok_t, const float* pos, const int32_t* text_len, void* stream) {
    if (!e || B <= 0 || ntok <= 0) return T5G_EINVAL;
    const t5g_config& c = e->c;
    if (B > c.max_batch || ntok > B * c.max_text) return T5G_ECAPACITY;
    hipStream_t st = (hipStream_t)stream;
    const int d = c.hidden, f = c.intermediate, D = c.head_dim;
    HIPCHK(hipMemcpyAsync(e->enc_len, text_len, B * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (e->text_max > 0) {
        // t5g_engine_set_text_max is a host hint that selects one-launch cross attention
        // over <= 64 keys: a stale hint below a row's real text length would silently
        // truncate that row's keys, so check it against the lengths once per call
        std::vector<int> lens(B);
        HIPCHK(hipMemcpyAsync(lens.data(), text_len, B * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b)
            if (lens[b] > e->text_max) {
                fprintf(stderr, "[t5gtts] text length %d of row %d > t5g_engine_set_text_max hint %d\n", lens[b], b,
                        e->text_max);
                return T5G_EINVAL;
            }
    }
    if (e->exact) return encode_exact(e, ntok, ids, tok_row, tok_t, pos, st);
    for (int l = 0; l < c.n_enc_layers; ++l) {
        const t5g_layer_weights& L = e->enc[l];
        NormArgs n = norm_args(ntok, d, c.rms_eps);
        if (l == 0) {
            n.ids = ids;
            n.table = (const bf16_t*)e->w.enc_embed;
            n.n_table = c.text_vocab;
            n.scale = c.normalizer;
        } else {
            n.delta = e->tmp;  // previous layer's down-proj output
            n.post_w = (const bf16_t*)e->enc[l - 1].norms[5];
            n.resid = e->h;
        }
        n.pre_w = (const bf16_t*)L.norms[0];
        n.resid_out = e->h;
        n.normed_out = e->xn;
        RC(resid_norm(n, st));
        RC(gemm(e->xn, d, ntok, L.qkv, e->qkv_dim, d, 1, nullptr, e->qkv, e->qkv_dim, EPI_BF16, st, true));
        RopeArgs r;
        memset(&r, 0, sizeof(r));
        r.X = e->qkv;
        r.ldx = e->qkv_dim;
        r.M = ntok;
        r.D = D;
        r.nq = c.n_heads;
        r.nk = c.n_kv_heads;
        r.nv = c.n_kv_heads;
        r.rope_q = r.rope_k = 1;
        r.pos = pos;
        r.inv_freq = e->w.inv_freq;
        r.tok_row = tok_row;
        r.tok_t = tok_t;
        r.Qout = e->q;
        r.ldq = e->q_dim;
        r.Kc = e->enc_k;
        r.Vc = e->enc_v;
        r.c_hstride = (long)c.max_text * D;
        r.c_bstride = r.c_hstride * c.n_kv_heads;
        RC(rope_store(r, st));
        RC(attn_packed(e, ntok, e->q, tok_row, tok_t, e->enc_k, e->enc_v, c.max_text, e->enc_len, 0,
                       c.enc_sliding[l] ? c.sliding_window : 0, e->att, st));
        RC(gemm(e->att, e->q_dim, ntok, L.o, d, e->q_dim, 1, nullptr, e->tmp, d, EPI_BF16, st, true));
        n = norm_args(ntok, d, c.rms_eps);
        n.delta = e->tmp;
        n.post_w = (const bf16_t*)L.norms[1];
        n.resid = e->h;
        n.pre_w = (const bf16_t*)L.norms[4];
        n.resid_out = e->h;
        n.normed_out = e->xn;
        RC(resid_norm(n, st));
        RC(gemm(e->xn, d, ntok, L.gate_up, 2 * f, d, 1, nullptr, e->act, f, EPI_GEGLU, st, true));
        RC(gemm(e->act, f, ntok, L.down, d, f, 1, nullptr, e->tmp, d, EPI_BF16, st, true));
    }
    // final: h + post_ff(down) -> encoder norm -> memory
    NormArgs n = norm_args(ntok, d, c.rms_eps);
    n.delta = e->tmp;
    n.post_w = (const bf16_t*)e->enc[c.n_enc_layers - 1].norms[5];
    n.resid = e->h;
    n.pre_w = (const bf16_t*)e->w.enc_final_norm;
    n.resid_out = e->h;
    n.normed_out = e->mem;
    RC(resid_norm(n, st));
    // cross-attention K/V of every decoder layer from memory (PM-RoPE on K)
    for (int l = 0; l < c.n_dec_layers; ++l) {
        RC(gemm(e->mem, d, ntok, e->dec[l].cross_kv, 2 * e->kv_dim, d, 1, nullptr, e->qkv, 2 * e->kv_dim,
                EPI_BF16, st, true));
        RopeArgs r;
        memset(&r, 0, sizeof(r));
        r.X = e->qkv;
        r.ldx = 2 * e->kv_dim;
        r.M = ntok;
        r.D = D;
        r.nk = c.n_kv_heads;
        r.nv = c.n_kv_heads;
        r.rope_k = 1;
        r.pos = pos;
        r.inv_freq = e->w.inv_freq;
        r.tok_row = tok_row;
        r.tok_t = tok_t;
        r.Kc = e->ck[l];
        r.Vc = e->cv[l];
        r.c_hstride = (long)c.max_text * D;
        r.c_bstride = r.c_hstride * c.n_kv_heads;
        RC(rope_store(r, st));
    }
    return T5G_OK;
}

DecGemmArgs dec_args(int M, const void* W, int N, int K, void* Y, int ldy, int nw) {
    DecGemmArgs g;
    memset(&g, 0, sizeof(g));
    g.M = M;
    g.K = K;
    g.W = (const bf16_t*)W;
    g.N = N;
    g.NG = ng_pad(N);
    g.KB = K / 32;
    g.Y = Y;
    g.ldy = ldy;
    g.nw = nw;
    g.splits = 1;
    return g;
}

// decode attention over a per-layer cache (self: the step's k/v appended in-kernel)
static int decode_attention(t5g_engine* e, int M, const bf16_t* K, const bf16_t* Vc, int cap, const int* kv_len,
                            int causal, int window, int q_col0, bool append, const float* pos, const float* tab,
                            int q_nsplit, int ldqp, hipStream_t st) {
    const t5g_config& c = e->c;
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.ldq = e->q_dim;
    a.Mq = M;
    a.K = K;
    a.V = Vc;
    a.kv_hstride = (long)cap * c.head_dim;
    a.kv_bstride = a.kv_hstride * c.n_kv_heads;
    a.kv_len = kv_len;
    a.Hkv = c.n_kv_heads;
    a.D = c.head_dim;
    a.G = c.n_heads / c.n_kv_heads;
    a.causal = causal;
    a.window = window;
    a.scale = c.attn_scale;
    a.softcap = c.softcap;   // eager checkpoints: the fast kernels apply the tanh softcap
    a.O = e->datt;
    a.ldo = e->q_dim;
    a.chunk = 64;
    a.nsplit = (cap + 63) / 64;
    if (append && e->audio_max > 0 && e->audio_max < cap) a.nsplit = (e->audio_max + 63) / 64;   // self: the call's rows
    a.kv_cap = cap;
    a.sbuf = e->asbuf;
    a.mbuf = e->ambuf;
    a.Qpart = e->part + q_col0;   // q columns of the projection's fp32 split-K slabs
    a.q_nsplit = q_nsplit;
    a.ldqp = ldqp;
    a.pos = pos;
    a.inv_freq = e->w.inv_freq;
    a.rope_tab = tab;
    a.append = append ? 1 : 0;
    a.k_col0 = e->q_dim - q_col0;
    a.v_col0 = e->q_dim + e->kv_dim - q_col0;
    a.flash = e->attn_flash ? 1 : 0;
    a.fpart = e->afpart;
    a.fstat = e->afstat;
    a.fticket = e->aftick;
    return attention_decode(a, st);
}

// the decode MLP half of decoder layer l as one persistent launch (fused.hip): cross-o
// slabs in e->part -> h / xn -> act -> down slabs in e->part; layer l's counter set
static FusedMlpArgs fused_mlp_fields(t5g_engine* e, int M, int l) {
    const t5g_config& c = e->c;
    const t5g_layer_weights& L = e->dec[l];
    FusedMlpArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.M = M;
    fa.d = c.hidden;
    fa.f = c.intermediate;
    fa.part_in = e->part;
    fa.post_w = (const bf16_t*)L.norms[3];
    fa.pre_w = (const bf16_t*)L.norms[4];
    fa.eps = c.rms_eps;
    fa.h = e->dh;
    fa.xn = e->dxn;
    fa.Wgu = (const bf16_t*)L.gate_up;
    fa.NGgu = ng_pad(2 * c.intermediate);
    fa.act = e->dact;
    fa.Wd = (const bf16_t*)L.down;
    fa.NGd = ng_pad(c.hidden);
    fa.part_out = e->part;
    fa.timeout = e->fsync;
    fa.sync = e->fsync + FM_LINE + (size_t)FM_SET_WORDS * l;
    fa.sync_next = e->fsync + FM_LINE + (size_t)FM_SET_WORDS * ((l + 1) % c.n_dec_layers);
    return fa;
}

static void p8_weight(const bf16_t*& W, const float*& S, const t5g_fp8_linear& x) {
    W = (const bf16_t*)x.p8;
    S = x.scale;
}

// FP8 mode with the MLP-half launch on (t5g_engine_set_fp8_mlp): gate/up and down are the
// Linears' P8 images with their row scales (fused_mlp_p8.hip)
FusedMlpArgs fused_args(t5g_engine* e, int M, int l) {
    FusedMlpArgs fa = fused_mlp_fields(e, M, l);
    if (e->fp8 && e->fp8_mlp) {
        fa.wfmt = 1;
        p8_weight(fa.Wgu, fa.sWgu, e->dec8[l].gate_up);
        p8_weight(fa.Wd, fa.sWd, e->dec8[l].down);
    }
    return fa;
}

// the same launch with the cross-attention chain in front (fused_kernels.h fused_block_kernel):
// o-proj slabs in e->part -> ... -> down slabs in e->part
FusedMlpArgs fused_block_args(t5g_engine* e, int M, int l) {
    const t5g_config& c = e->c;
    const t5g_layer_weights& L = e->dec[l];
    FusedMlpArgs fa = fused_mlp_fields(e, M, l);
    fa.xattn = 1;
    fa.o_slabs = e->part;
    fa.post1_w = (const bf16_t*)L.norms[1];
    fa.pre1_w = (const bf16_t*)L.norms[2];
    fa.xn1 = e->dhh;
    fa.Wq = (const bf16_t*)L.cross_q;
    fa.NGq = ng_pad(e->q_dim);
    fa.qslab = e->part2;
    fa.ck = e->ck[l];
    fa.cv = e->cv[l];
    fa.kv_cap = c.max_text;
    fa.text_max = e->text_max > 0 ? e->text_max : c.max_text;
    fa.enc_len = e->enc_len;
    fa.rope_tab = e->rope_tab;
    fa.q_dim = e->q_dim;
    fa.Hq = c.n_heads;
    fa.Hkv = c.n_kv_heads;
    fa.D = c.head_dim;
    fa.scale = c.attn_scale;
    fa.softcap = c.softcap;
    fa.att = e->datt2;
    fa.Wo = (const bf16_t*)L.cross_o;
    fa.NGo = ng_pad(c.hidden);
    fa.oslab = e->part2 + (size_t)2 * M * e->q_dim;
    fa.dslab = fa.oslab + (size_t)4 * M * c.hidden;
    fa.post3_w = (const bf16_t*)L.norms[5];
    const bool last = l == c.n_dec_layers - 1;
    fa.pre3_w = (const bf16_t*)(last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]);
    fa.Wqkv = last ? nullptr : (const bf16_t*)e->dec[l + 1].qkv;
    fa.NGqkv = ng_pad(e->qkv_dim);
    fa.qkv_dim = e->qkv_dim;
    fa.qkv_out = e->part;
    fa.att_self = e->datt;
    fa.Wo1 = (const bf16_t*)L.o;
    fa.o1slab = fa.dslab + (size_t)8 * M * c.hidden;
    // FP8 mode with the whole-layer launch on (t5g_engine_set_fp8_block): every weight of the
    // launch is the Linear's P8 image with its row scales (fused_p8.hip; no mixed launch)
    if (e->fp8 && e->fp8_block) {
        const t5g_fp8_layer& P = e->dec8[l];
        fa.wfmt = 1;
        p8_weight(fa.Wo1, fa.sWo1, P.o);
        p8_weight(fa.Wq, fa.sWq, P.cross_q);
        p8_weight(fa.Wo, fa.sWo, P.cross_o);
        p8_weight(fa.Wgu, fa.sWgu, P.gate_up);
        p8_weight(fa.Wd, fa.sWd, P.down);
        if (!last) p8_weight(fa.Wqkv, fa.sWqkv, e->dec8[l + 1].qkv);
    }
    return fa;
}

// stage S (fast path): layer l's flash decode self-attention inside the launch, with
// decode_attention's arguments (the cache, the call's chunk grid, the q|k|v slabs)
static void fused_s_fields(t5g_engine* e, int l, FusedMlpArgs& fa) {
    const t5g_config& c = e->c;
    fa.qkv_in = e->part;
    fa.sk = e->sk[l];
    fa.sv = e->sv[l];
    fa.s_cap = c.max_audio;
    fa.s_nsplit = (c.max_audio + 63) / 64;
    if (e->audio_max > 0 && e->audio_max < c.max_audio) fa.s_nsplit = (e->audio_max + 63) / 64;
    fa.kv_len = e->kv_len;
    fa.window = c.dec_sliding[l] ? c.sliding_window : 0;
    fa.fpart = e->afpart;
    fa.fstat = e->afstat;
    fa.fticket = e->aftick;
}

// stage S at the end (fast path, attn_in_block 2): launch l projects layer l + 1's q|k|v,
// runs its self attention and its o-projection into the o1slab region, which the next
// launch's N1 reads as o_slabs (layer 0's come from the step's prologue in e->part);
// false when the launch is not built for them
bool fused_block_tail(t5g_engine* e, int l, FusedMlpArgs& fa) {
    const t5g_config& c = e->c;
    fa.Wo1 = nullptr;   // the o-projection of this layer ran at the end of the previous launch
    fa.sWo1 = nullptr;
    fa.o_slabs = l == 0 ? e->part : fa.o1slab;
    if (l == c.n_dec_layers - 1) return fused_mlp_check(fa) == 0;
    fused_s_fields(e, l + 1, fa);
    fa.self_tail = 1;
    fa.Wo1n = (const bf16_t*)e->dec[l + 1].o;
    if (fa.wfmt) p8_weight(fa.Wo1n, fa.sWo1n, e->dec8[l + 1].o);
    fa.o1n = fa.o1slab;
    fa.att_self = e->datt;
    return fused_mlp_check(fa) == 0;
}

// stage S in front of layer l's o-projection; false when the launch is not built for it (the
// attention then runs as its own launch)
static bool fused_block_self(t5g_engine* e, int l, FusedMlpArgs& fa) {
    // mode 1, or mode 2 on a call the tail does not take (2 slots per worker): S in front
    if (e->attn_in_block < 1 || !e->attn_flash || !fa.Wo1) return false;
    fa.self_attn = 1;
    fused_s_fields(e, l, fa);
    return fused_mlp_check(fa) == 0;
}

DecodePlan decode_plan(t5g_engine* e, int M, int block_rows, bool switches) {
    const t5g_config& c = e->c;
    // the 2b-2b widths, each named by the Linears whose K or N it is
    const bool wd = c.hidden == 2304, wf = c.intermediate == 9216, wq = e->q_dim == 2048;
    const bool rows32 = M <= 32;   // the register-X GEMVs and the MLP-half launch: two 16-row tiles
    const GemvSite gemm_only = {0, 0, 0, false};
    DecodePlan p;
    // register-X GEMVs, so a row's sums never depend on the batch. q|k|v and cross-q: 12 waves
    // over 2 k-slices of 36 k-steps (the fused block's QKV / Q stages); o and cross-o: 4 slices
    // of 16 k-steps (tools/probe_proj_rx.py: 4.13 vs 4.23 us at 8 rows, 5.2 vs 6.8 at 32);
    // down: 36-k-step slices, 32 blocks per slice (tools/probe_down_rx.py: 11.2 vs 16.3 us at
    // 32 rows, 9.0 vs 9.4 at 8)
    p.qkv = rows32 && wd ? GemvSite{12, e->s_qkv, 0, true} : gemm_only;
    p.proj = rows32 && wd && wq ? GemvSite{8, e->s_o, 0, true} : gemm_only;
    p.cross_q = rows32 && wd && wq ? GemvSite{12, 2, 0, true} : gemm_only;
    p.down = rows32 && wd && wf ? GemvSite{12, e->s_down, 0, true} : gemm_only;
    // gate/up on the one-block-per-CU GEMV; register-X at the 2b-2b width, every unit's weights
    // requested up front (18.84 -> 18.39 us at 8 rows, 24.2 -> 23.9 at 32, bitwise equal:
    // tools/probe_rx_all.py)
    p.gate_up = rows32 && wd ? GemvSite{12, 1, -1, true} : M <= 16 ? GemvSite{8, 1, 8, false} : gemm_only;
    p.mlp_half = e->fused_mlp && rows32 && wd && wf && c.n_dec_layers >= 2;
    p.block = M <= block_rows && (!switches || (p.mlp_half && wq));
    // FP8 mode: the whole-layer launch has a P8 form for one tile only, behind its own switch
    // (t5g_engine_set_fp8_block; block_rows above 16 does not apply); the MLP-half launch has
    // one for both tile counts, behind its own switch too (t5g_engine_set_fp8_mlp). Everything
    // else runs the per-op launches on the P8 GEMVs.
    if (e->fp8) {
        p.block = p.block && e->fp8_block && M <= 16;
        p.mlp_half = p.mlp_half && e->fp8_mlp;
    }
    // stage S at the end of the launches (attn_in_block 2): every layer's launch must take it
    p.tail = p.block && e->attn_in_block == 2 && (!switches || e->attn_flash);
    for (int l = 0; l < c.n_dec_layers && p.tail; ++l) {
        FusedMlpArgs fa = fused_block_args(e, M, l);
        p.tail = fused_block_tail(e, l, fa);
    }
    return p;
}

DecodeLaunch decode_layer_launch(t5g_engine* e, const DecodePlan& p, int M, int l, FusedMlpArgs& fa) {
    if (p.block) {
        fa = fused_block_args(e, M, l);
        if (fused_mlp_check(fa) == 0) {
            FusedMlpArgs s = fa;   // fa stays the launch without S when S is refused
            if (!fused_block_self(e, l, s)) return DL_BLOCK;
            fa = s;
            return DL_BLOCK_S;
        }
    }
    if (!p.mlp_half) return DL_PER_OP;
    fa = fused_args(e, M, l);
    return DL_MLP_HALF;
}

// layer 0's input: the embedded tokens, normed for the self attention
static NormArgs embed_norm_args(const t5g_engine* e, int M, const int* ids, bf16_t* h, bf16_t* xn) {
    const t5g_config& c = e->c;
    NormArgs n = norm_args(M, c.hidden, c.rms_eps);
    n.ids = ids;
    n.table = (const bf16_t*)e->w.audio_embed;
    n.n_table = c.n_audio_tokens;
    n.scale = c.normalizer;
    n.pre_w = (const bf16_t*)e->dec[0].norms[0];
    n.resid_out = h;
    n.normed_out = xn;
    return n;
}

// One decoder pass over M packed tokens (prefill): tiled GEMMs with bf16 outputs, RoPE and the
// cache stores in rope_store, packed attention.
static int prefill_pass(t5g_engine* e, int M, const int* ids, const int* tok_row, const int* tok_t, const float* pos,
                        hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate, D = c.head_dim;
    // a Linear into tmp, then h = h + RMSNorm_post(tmp), xn = RMSNorm_pre(h)
    auto linear = [&](const bf16_t* x, int K, const void* W) -> int {
        return gemm(x, K, M, W, d, K, 1, nullptr, e->tmp, d, EPI_BF16, st, true);
    };
    auto resid = [&](const void* post_w, const void* pre_w) -> int {
        NormArgs n = norm_args(M, d, c.rms_eps);
        n.delta = e->tmp;
        n.post_w = (const bf16_t*)post_w;
        n.resid = e->h;
        n.pre_w = (const bf16_t*)pre_w;
        n.resid_out = e->h;
        n.normed_out = e->xn;
        return resid_norm(n, st);
    };
    auto rope_args = [&]() {
        RopeArgs r;
        memset(&r, 0, sizeof(r));
        r.M = M;
        r.D = D;
        r.pos = pos;
        r.inv_freq = e->w.inv_freq;
        r.tok_row = tok_row;
        r.tok_t = tok_t;
        r.kv_len = e->kv_len;
        r.Qout = e->q;
        r.ldq = e->q_dim;
        return r;
    };
    RC(resid_norm(embed_norm_args(e, M, ids, e->h, e->xn), st));
    for (int l = 0; l < c.n_dec_layers; ++l) {
        const t5g_layer_weights& L = e->dec[l];
        const bool last = l == c.n_dec_layers - 1;
        // --- self attention
        RC(gemm(e->xn, d, M, L.qkv, e->qkv_dim, d, 1, nullptr, e->qkv, e->qkv_dim, EPI_BF16, st, true));
        RopeArgs r = rope_args();
        r.X = e->qkv;
        r.ldx = e->qkv_dim;
        r.nq = c.n_heads;
        r.nk = r.nv = c.n_kv_heads;
        r.rope_q = r.rope_k = 1;
        r.Kc = e->sk[l];
        r.Vc = e->sv[l];
        r.c_hstride = (long)c.max_audio * D;
        r.c_bstride = r.c_hstride * c.n_kv_heads;
        RC(rope_store(r, st));
        RC(attn_packed(e, M, e->q, tok_row, tok_t, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1,
                       c.dec_sliding[l] ? c.sliding_window : 0, e->att, st));
        RC(linear(e->att, e->q_dim, L.o));
        RC(resid(L.norms[1], L.norms[2]));
        // --- PM cross attention (q rotated by the decoder progress, :149-165)
        RC(gemm(e->xn, d, M, L.cross_q, e->q_dim, d, 1, nullptr, e->q, e->q_dim, EPI_BF16, st, true));
        r = rope_args();
        r.X = e->q;
        r.ldx = e->q_dim;
        r.nq = c.n_heads;
        r.rope_q = 1;
        RC(rope_store(r, st));
        RC(attn_packed(e, M, e->q, tok_row, tok_t, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, e->att, st));
        RC(linear(e->att, e->q_dim, L.cross_o));
        RC(resid(L.norms[3], L.norms[4]));
        // --- GeGLU MLP
        RC(gemm(e->xn, d, M, L.gate_up, 2 * f, d, 1, nullptr, e->act, f, EPI_GEGLU, st, true));
        RC(linear(e->act, f, L.down));
        RC(resid(L.norms[5], last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]));
    }
    return T5G_OK;
}

// A decode Linear at one of the plan's sites: on the GEMV when the site has one, on the tiled
// GEMM (gemm_splits k-slices) otherwise or when the GEMV reports -1 (its per-block LDS does
// not fit this device's CU count, e.g. a CPX partition). *on_gemv: which of the two ran.
// w8 (FP8 mode, register-X sites only): the P8 image + row scales of the same Linear; the GEMV
// streams those, the GEMM fallback the P16 image of W_q.
static int rx_or_gemm(const GemvSite& gv, int gemm_splits, const bf16_t* X, int M, const void* W, int N, int K,
                      void* Y, int ldy, int epi, hipStream_t st, bool* on_gemv = nullptr,
                      const t5g_fp8_linear* w8 = nullptr) {
    if (on_gemv) *on_gemv = false;
    if (gv.nw) {
        const bool p8 = w8 && w8->p8 && gv.rx;
        DecGemmArgs g = dec_args(M, p8 ? w8->p8 : W, N, K, Y, ldy, gv.nw);
        g.X = X;
        g.ldx = K;
        g.splits = gv.splits;
        g.un = gv.un;
        g.layout_rx = gv.rx;
        const int rc = p8 ? gemv_rx_p8(g, w8->scale, epi, st) : gemv_dec(g, epi, st);
        if (rc != -1) {
            if (on_gemv) *on_gemv = rc == 0;
            return rc;
        }
    }
    return gemm(X, K, M, W, N, K, gemm_splits, nullptr, Y, ldy, epi, st);
}

// One decoder step over the M rows fed by the sampler buffers (tokens, positions, lengths):
// every Linear writes fp32 split-K slabs into e->part that the next launch sums (spreading
// the weight streams over >= 512 blocks); decode_plan says which launches a layer runs.
// Eager checkpoints (softcap > 0) take the same launches: the attention kernels apply the
// tanh softcap in the score (common.h fast_score).
static int decode_pass(t5g_engine* e, int M, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate;
    constexpr int s_qkv = t5g_engine::s_qkv, s_o = t5g_engine::s_o, s_down = t5g_engine::s_down;
    const float* pos = e->next_pos;
    // one cos/sin table per step: every layer's q/k rotation uses the same positions
    // (written by layer 0's embedding-norm launch below)
    const float* tab = e->rope_tab;
    const DecodePlan p = decode_plan(e, M, e->block_max_rows);
    // norm after a Linear: h = h + RMSNorm_post(sum of the slabs), xn = RMSNorm_pre(h)
    auto resid = [&](int splits, const void* post_w, const void* pre_w) -> int {
        NormArgs n = norm_args(M, d, c.rms_eps);
        n.part = e->part;
        n.nsplit = splits;
        n.ldp = d;
        n.post_w = (const bf16_t*)post_w;
        n.resid = e->dh;
        n.pre_w = (const bf16_t*)pre_w;
        n.resid_out = e->dh;
        n.normed_out = e->dxn;
        return resid_norm(n, st);
    };
    // self attention over layer l's cache: q rotated, k rotated + appended inside the launch
    auto self_attention = [&](int l) -> int {
        return decode_attention(e, M, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1,
                                c.dec_sliding[l] ? c.sliding_window : 0, 0, true, pos, tab, s_qkv, e->qkv_dim, st);
    };
    // attention output projection into the norm's slabs
    auto out_proj = [&](const void* W, const t5g_fp8_linear* w8) -> int {
        return rx_or_gemm(p.proj, s_o, e->datt, M, W, d, e->q_dim, e->part, d, EPI_F32, st, nullptr, w8);
    };
    NormArgs n0 = embed_norm_args(e, M, e->next_token, e->dh, e->dxn);
    n0.rope_pos = pos;   // and the step's RoPE table, in the same launch
    n0.rope_inv_freq = e->w.inv_freq;
    n0.rope_tab = e->rope_tab;
    n0.rope_D = c.head_dim;
    e->s_mode_used = p.tail ? 2 : 0;
    RC(resid_norm(n0, st));
    bool qkv_done = false;   // the previous layer's fused block projected this layer's q|k|v
    for (int l = 0; l < c.n_dec_layers; ++l) {
        const t5g_layer_weights& L = e->dec[l];
        const t5g_fp8_layer* L8 = e->fp8 ? &e->dec8[l] : nullptr;   // FP8 mode: the layer's P8 images
        const bool last = l == c.n_dec_layers - 1;
        if (!qkv_done)
            RC(rx_or_gemm(p.qkv, s_qkv, e->dxn, M, L.qkv, e->qkv_dim, d, e->part, e->qkv_dim, EPI_F32, st, nullptr,
                          L8 ? &L8->qkv : nullptr));
        qkv_done = false;
        FusedMlpArgs fa;
        if (p.tail) {
            // layer 0's attention and o-projection as their own launches (the step's
            // prologue), then every layer's launch runs the next layer's attention and
            // o-projection at its end (bitwise equal to the launches below)
            if (l == 0) {
                RC(self_attention(l));
                RC(out_proj(L.o, L8 ? &L8->o : nullptr));
            }
            fa = fused_block_args(e, M, l);
            if (!fused_block_tail(e, l, fa)) return T5G_EUNSUPPORTED;   // the plan checked every layer
            RC(fused_mlp(fa, st));
            ++e->blk_launches;
            if (!last) ++e->s_launches;
            qkv_done = true;
            continue;
        }
        const DecodeLaunch launch = decode_layer_launch(e, p, M, l, fa);
        // the rest of the layer (o-projection, cross attention, MLP half, the last norm and the
        // next layer's q|k|v) as one persistent launch (fused_kernels.h fused_block_kernel), with the
        // attention as its stage S in front or as its own launch before it (all three bitwise
        // equal to the per-op launches below)
        if (launch == DL_BLOCK_S || launch == DL_BLOCK) {
            if (launch == DL_BLOCK) RC(self_attention(l));
            RC(fused_mlp(fa, st));
            ++e->blk_launches;
            if (launch == DL_BLOCK_S) {
                ++e->s_launches;
                e->s_mode_used = 1;
            }
            qkv_done = !last;
            continue;
        }
        RC(self_attention(l));
        RC(out_proj(L.o, L8 ? &L8->o : nullptr));
        RC(resid(s_o, L.norms[1], L.norms[2]));
        // --- PM cross attention (q rotated by the decoder progress, :149-165); the GEMM
        // fallback of cross-q writes s_o slabs, the GEMV its own two
        bool q_gemv = false;
        RC(rx_or_gemm(p.cross_q, s_o, e->dxn, M, L.cross_q, e->q_dim, d, e->part, e->q_dim, EPI_F32, st, &q_gemv,
                      L8 ? &L8->cross_q : nullptr));
        RC(decode_attention(e, M, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, 0, false, pos, tab,
                            q_gemv ? p.cross_q.splits : s_o, e->q_dim, st));
        RC(out_proj(L.cross_o, L8 ? &L8->cross_o : nullptr));
        // --- norm + GeGLU MLP as one persistent launch (fused.hip; bitwise equal to the three
        // launches below); -1: a shape / device the launch is not built for
        const int rc = launch == DL_MLP_HALF ? fused_mlp(fa, st) : -1;
        if (rc == 0) ++e->mlp_launches;
        if (rc != 0) {
            if (rc != -1) RC(rc);
            RC(resid(s_o, L.norms[3], L.norms[4]));
            RC(rx_or_gemm(p.gate_up, 1, e->dxn, M, L.gate_up, 2 * f, d, e->dact, f, EPI_GEGLU, st, nullptr,
                          L8 ? &L8->gate_up : nullptr));
            RC(rx_or_gemm(p.down, s_down, e->dact, M, L.down, d, f, e->part, d, EPI_F32, st, nullptr,
                          L8 ? &L8->down : nullptr));
        }
        RC(resid(s_down, L.norms[5], last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]));
    }
    return T5G_OK;
}

// one decoder step + predict head for the e->B rows fed by the sampler buffers
static int head(t5g_engine* e, const bf16_t* xn_rows, int B, hipStream_t st);
static int head_exact(t5g_engine* e, const bf16_t* xn_rows16, int B, hipStream_t st);
int decode_forward(t5g_engine* e, hipStream_t st) {
    if (e->exact) {
        RC(decoder_pass_exact(e, e->B, e->next_token, nullptr, nullptr, e->next_pos, true, st));
        return head_exact(e, e->dxn16, e->B, st);
    }
    int rc = decode_pass(e, e->B, st);
    if (rc) return rc;
    return head(e, e->dxn, e->B, st);
}

static int head(t5g_engine* e, const bf16_t* xn_rows, int B, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden;
    RC(gemm(xn_rows, d, B, e->w.head1, d, d, 1, e->w.head1_bias, e->dhh, d, EPI_BIAS_GELU, st));
    if (B <= 32 && d == 2304) {
        // 65,541-row head on the register-resident-X GEMV (tools/probe_head_nw.py: 50.3 vs
        // 56.3 us at 8 rows, 58.6 vs 103.1 at 32). 4 waves at every batch size: above 16 rows
        // only 4 waves' partial sums (17 units x 2 tiles x 4 waves x 1 KiB) fit LDS, and one
        // wave count keeps a row's logits independent of the batch
        // FP8 mode: the same launch on head2's P8 image
        DecGemmArgs g = dec_args(B, e->fp8 ? e->head2_8.p8 : e->w.head2, e->V, d, e->logits, e->logits_ld, 4);
        g.X = e->dhh;
        g.ldx = d;
        g.un = 8;
        g.layout_rx = 1;
        g.bias = (const bf16_t*)e->w.head2_bias;
        const int rc = e->fp8 ? gemv_rx_p8(g, e->head2_8.scale, EPI_BIAS_BF16, st) : gemv_dec(g, EPI_BIAS_BF16, st);
        if (rc == -1)
            RC(gemm(e->dhh, d, B, e->w.head2, e->V, d, 1, e->w.head2_bias, e->logits, e->logits_ld, EPI_BIAS_BF16, st));
        else RC(rc);
    } else {
        RC(gemm(e->dhh, d, B, e->w.head2, e->V, d, 1, e->w.head2_bias, e->logits, e->logits_ld, EPI_BIAS_BF16, st));
    }
    return T5G_OK;
}

extern "C" int t5g_prefill(t5g_engine* e, int32_t B, int32_t ntok, const int32_t* ids, const int32_t* tok_row,
                           const int32_t* tok_t, const float* pos, const int32_t* kv_len,
                           const int32_t* last_index, void* stream) {
    if (!e || B <= 0 || ntok <= 0) return T5G_EINVAL;
    const t5g_config& c = e->c;
    if (B > c.max_batch || ntok > B * c.max_audio) return T5G_ECAPACITY;
    hipStream_t st = (hipStream_t)stream;
    if (e->audio_max > 0) {
        // t5g_engine_set_audio_max is a host hint that sizes the decode attention grids (and
        // the stop rule): a stale hint below a row's length would silently drop that row's
        // keys and leave the flash tickets counting, so check it once per call
        std::vector<int> lens(B);
        HIPCHK(hipMemcpyAsync(lens.data(), kv_len, B * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b)
            if (lens[b] > e->audio_max) {
                fprintf(stderr, "[t5gtts] prefill length %d of row %d > t5g_engine_set_audio_max hint %d\n", lens[b],
                        b, e->audio_max);
                return T5G_EINVAL;
            }
    }
    e->B = B;
    HIPCHK(hipMemcpyAsync(e->kv_len, kv_len, B * sizeof(int), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(e->last_rows, last_index, B * sizeof(int), hipMemcpyDeviceToDevice, st));
    int rc = e->exact ? decoder_pass_exact(e, ntok, ids, tok_row, tok_t, pos, false, st)
                      : prefill_pass(e, ntok, ids, tok_row, tok_t, pos, st);
    if (rc) return rc;
    // the pass's last norm wrote final-normed hidden of every token into xn;
    // gather each row's last token
    NormArgs n = norm_args(B, c.hidden, c.rms_eps);
    // copy rows: reuse resid_norm as a gather (delta = xn, no norms)
    n.delta = e->xn;
    n.out_rows = e->last_rows;
    n.resid_out = e->dxn;
    RC(resid_norm(n, st));
    if (e->exact) {
        RC(to_x16(e->dxn, c.hidden, B, c.hidden, e->dxn16, st));
        return head_exact(e, e->dxn16, B, st);
    }
    return head(e, e->dxn, B, st);
}

extern "C" int t5g_sampler_setup(t5g_engine* e, int32_t B, const t5g_sampler_row* rows, const t5g_sampler_state* init,
                                 const int32_t* top_k_list, int32_t n_top_k_list, const int32_t* silence,
                                 int32_t n_silence, const void* noise, int32_t noise_steps, void* stream) {
    if (!e || B <= 0 || B > e->c.max_batch || !rows || !init) return T5G_EINVAL;
    if (n_top_k_list > 4096 || n_silence > 4096) return T5G_ECAPACITY;
    static_assert(sizeof(t5g_sampler_row) == sizeof(SamplerRow), "row layout");
    static_assert(sizeof(t5g_sampler_state) == sizeof(SamplerState), "state layout");
    // the decode grids cover the call's key bound (t5g_engine_set_audio_max); a row already
    // past it would append keys no launch reads
    const int bound = e->audio_max > 0 ? e->audio_max : e->c.max_audio;
    for (int b = 0; b < B; ++b)
        if (init[b].current_length < 0 || init[b].current_length > bound) {
            fprintf(stderr, "[t5gtts] row %d current_length %d outside the call's key bound %d\n", b,
                    init[b].current_length, bound);
            return T5G_EINVAL;
        }
    // the sampler kernels index the shared lists with each row's offsets and edit the logit
    // of prev_token unchecked: every row's ranges must lie inside what this call uploads
    if (n_top_k_list < 0 || n_silence < 0 || (n_top_k_list > 0 && !top_k_list) || (n_silence > 0 && !silence))
        return T5G_EINVAL;
    for (int b = 0; b < B; ++b) {
        const t5g_sampler_row& r = rows[b];
        const bool bad_silence = r.silence_off < 0 || r.n_silence < 0 ||
                                 (r.n_silence > 0 && (int64_t)r.silence_off + r.n_silence > n_silence);
        const bool bad_top_k = r.top_k_list_off < 0 || r.top_k_list_len < 0 ||
                               (r.top_k_list_len > 0 && (int64_t)r.top_k_list_off + r.top_k_list_len > n_top_k_list);
        if (bad_silence || bad_top_k || init[b].prev_token >= e->V) {
            fprintf(stderr, "[t5gtts] row %d: silence [%d, +%d) of %d, top-k list [%d, +%d) of %d, prev_token %d of %d\n",
                    b, r.silence_off, r.n_silence, n_silence, r.top_k_list_off, r.top_k_list_len, n_top_k_list,
                    init[b].prev_token, e->V);
            return T5G_EINVAL;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    e->B = B;
    e->decode_state_invalid = false;
    HIPCHK(hipMemcpyAsync(e->rows, rows, B * sizeof(SamplerRow), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->state, init, B * sizeof(SamplerState), hipMemcpyHostToDevice, st));
    if (n_top_k_list > 0)
        HIPCHK(hipMemcpyAsync(e->topk_list, top_k_list, n_top_k_list * sizeof(int), hipMemcpyHostToDevice, st));
    if (n_silence > 0)
        HIPCHK(hipMemcpyAsync(e->silence, silence, n_silence * sizeof(int), hipMemcpyHostToDevice, st));
    if (e->noise != (const bf16_t*)noise || e->noise_steps != noise_steps) {
        // noise pointer is baked into the captured graphs
        drop_graphs(e);
    }
    e->noise = (const bf16_t*)noise;
    e->noise_steps = noise_steps;
    HIPCHK(hipMemsetAsync(e->out_tokens, 0xff, (size_t)B * e->c.max_gen * sizeof(int), st));
    return T5G_OK;
}

extern "C" int t5g_engine_set_noise_mt(t5g_engine* e, const uint32_t* raw, int32_t steps) {
    if (!e || (raw && steps <= 0)) return T5G_EINVAL;
    if (!raw) steps = 0;
    if (e->noise_mt != raw || e->noise_mt_steps != steps) drop_graphs(e);   // baked into the captured graphs
    e->noise_mt = raw;
    e->noise_mt_steps = steps;
    return T5G_OK;
}

static SamplerArgs sampler_args(t5g_engine* e, const bf16_t* logits, int ld, int B) {
    SamplerArgs s;
    memset(&s, 0, sizeof(s));
    s.logits = logits;
    s.ldl = ld;
    s.V = e->V;
    s.B = B;
    s.rows = e->rows;
    s.state = e->state;
    s.top_k_list = e->topk_list;
    s.silence = e->silence;
    s.noise = e->noise;
    s.noise_steps = e->noise_steps;
    s.noise_mt = e->noise_mt;
    s.noise_mt_steps = e->noise_mt_steps;
    s.eos = e->c.eos;
    s.eos_guard = e->c.eos_guard;
    s.budget_extra = e->c.budget_extra;
    s.text_guard = e->c.text_guard;
    s.progress_scale = e->c.progress_scale;
    s.out_tokens = e->out_tokens;
    s.max_gen = e->c.max_gen;
    // rows are force-stopped at the call's key bound (the decode attention grid covers
    // exactly that many keys); the host sets it at or above every row's prompt + budget,
    // so it never stops a row the reference would have run on
    s.max_len = e->audio_max > 0 ? e->audio_max : e->c.max_audio;
    s.kv_len = e->kv_len;
    s.next_pos = e->next_pos;
    s.next_token = e->next_token;
    s.flags = e->flags;
    s.fs_val = e->fs_val;
    s.fs_idx = e->fs_idx;
    s.fs_cnt = e->fs_cnt;
    s.fs_amv = e->fs_amv;
    s.fs_ami = e->fs_ami;
    s.fs_ticket = e->fs_ticket;
    s.fs_slow = e->fast_sampler ? e->fs_slow : nullptr;
    return s;
}

static int decode_iter(t5g_engine* e, hipStream_t st) {
    const int B = e->B;
    RC(sample(sampler_args(e, e->logits, e->logits_ld, B), st));
    return decode_forward(e, st);
}

extern "C" int t5g_decode(t5g_engine* e, int32_t n_steps, int32_t use_graph, void* stream) {
    if (!e || e->B <= 0) return T5G_EINVAL;
    if (e->decode_state_invalid) {
        fprintf(stderr, "[t5gtts] t5g_decode after a timing hook: start a new call (t5g_prefill + t5g_sampler_setup)\n");
        return T5G_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (!use_graph) {
        for (int i = 0; i < n_steps; ++i) {
            int rc = decode_iter(e, st);
            if (rc) return rc;
        }
        return T5G_OK;
    }
    if (!e->gexec || e->graph_B != e->B) {
        drop_graphs(e);
        for (int which = 0; which < 2; ++which) {
            auto iters = [&](hipStream_t cs) {
                int rc = T5G_OK;
                for (int i = 0; i < (which ? GRAPH_STEPS : 1) && !rc; ++i) rc = decode_iter(e, cs);
                return rc;
            };
            const int rc = capture(e, iters, which ? &e->graph_n : &e->graph, which ? &e->gexec_n : &e->gexec);
            if (rc) {
                drop_graphs(e);   // never a one-step graph without its GRAPH_STEPS twin
                return rc;
            }
        }
        e->graph_B = e->B;
    }
    int i = 0;
    for (; i + GRAPH_STEPS <= n_steps; i += GRAPH_STEPS) HIPCHK(hipGraphLaunch(e->gexec_n, st));
    for (; i < n_steps; ++i) HIPCHK(hipGraphLaunch(e->gexec, st));
    return T5G_OK;
}

extern "C" int t5g_read_state(t5g_engine* e, t5g_sampler_state* out, int32_t B, void* stream) {
    if (!e || !out || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, e->state, B * sizeof(SamplerState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return T5G_OK;
}

// The fused launches' sticky timeout word: non-zero when an in-launch hand-off gave up
// (outputs of those launches invalid). Cleared with the counters; T5G_EHANDOFF then.
int check_handoff(t5g_engine* e, hipStream_t st) {
    unsigned tmo = 0;
    HIPCHK(hipMemcpyAsync(&tmo, e->fsync, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!tmo) return T5G_OK;
    fprintf(stderr, "[t5gtts] fused decode hand-off timed out (code %u)\n", tmo);
    hipMemsetAsync(e->fsync, 0, fsync_words(e->c) * sizeof(unsigned), st);
    // the flash / stage-S arrival tickets are zero between launches; a launch that gave up
    // (or left chunks uncovered) can leave them counting, so they are cleared with the counters
    hipMemsetAsync(e->aftick, 0, (size_t)e->c.max_batch * e->c.n_kv_heads * sizeof(unsigned), st);
    hipStreamSynchronize(st);
    return T5G_EHANDOFF;
}

extern "C" int t5g_read_tokens(t5g_engine* e, int32_t* out, int32_t B, void* stream) {
    if (!e || !out || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, e->out_tokens, (size_t)B * e->c.max_gen * sizeof(int), hipMemcpyDeviceToHost, st));
    // an in-launch hand-off of the fused launch gave up waiting (a workgroup was not
    // resident): the outputs are garbage; the counters are cleared for the next call
    return check_handoff(e, st);
}

extern "C" int t5g_engine_poison_handoff(t5g_engine* e, uint32_t code) {
    if (!e || !code || !e->fsync) return T5G_EINVAL;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(e->fsync, &code, sizeof(unsigned), hipMemcpyHostToDevice));
    HIPCHK(hipDeviceSynchronize());
    return T5G_OK;
}

extern "C" int t5g_engine_set_attn_flash(t5g_engine* e, int32_t enable) {
    if (!e) return T5G_EINVAL;
    if (e->attn_flash != (enable != 0)) {
        e->attn_flash = enable != 0;
        drop_graphs(e);   // captured launches follow the flag
    }
    return T5G_OK;
}

extern "C" int t5g_engine_set_attn_in_block(t5g_engine* e, int32_t mode) {
    if (!e || mode < 0 || mode > 2) return T5G_EINVAL;
    if (e->attn_in_block != mode) {
        e->attn_in_block = mode;
        drop_graphs(e);   // captured launches follow the flag
    }
    return T5G_OK;
}

extern "C" int t5g_engine_attn_in_block_mode(t5g_engine* e, int32_t* mode) {
    if (!e || !mode) return T5G_EINVAL;
    *mode = e->s_mode_used;
    return T5G_OK;
}

extern "C" int t5g_engine_attn_in_block_launches(t5g_engine* e, int64_t* n) {
    if (!e || !n) return T5G_EINVAL;
    *n = e->s_launches;
    return T5G_OK;
}

extern "C" int t5g_engine_block_launches(t5g_engine* e, int64_t* n) {
    if (!e || !n) return T5G_EINVAL;
    *n = e->blk_launches;
    return T5G_OK;
}

extern "C" int t5g_engine_mlp_half_launches(t5g_engine* e, int64_t* n) {
    if (!e || !n) return T5G_EINVAL;
    *n = e->mlp_launches;
    return T5G_OK;
}

extern "C" int t5g_engine_set_block_max_rows(t5g_engine* e, int32_t n) {
    if (!e || (n != 16 && n != 32)) return T5G_EINVAL;
    if (e->block_max_rows != n) {
        e->block_max_rows = n;
        drop_graphs(e);   // captured launches follow the limit
    }
    return T5G_OK;
}

extern "C" int t5g_engine_set_text_max(t5g_engine* e, int32_t n) {
    if (!e || n < 0 || n > e->c.max_text) return T5G_EINVAL;
    const int before = e->text_max > 0 ? e->text_max : e->c.max_text;
    const int after = n > 0 ? n : e->c.max_text;
    if ((before <= 64) != (after <= 64)) drop_graphs(e);   // the decode layout baked into the graphs follows it
    e->text_max = n;
    return T5G_OK;
}

extern "C" int t5g_engine_set_audio_max(t5g_engine* e, int32_t n) {
    if (!e || n < 0 || n > e->c.max_audio) return T5G_EINVAL;
    const int before = e->audio_max > 0 ? e->audio_max : e->c.max_audio;
    const int after = n > 0 ? n : e->c.max_audio;
    if ((before + 63) / 64 != (after + 63) / 64 || before != after) drop_graphs(e);   // grid + stop rule in the graphs
    e->audio_max = n;
    return T5G_OK;
}

extern "C" int t5g_engine_xlayer_launches(t5g_engine* e, int64_t* n) {
    if (!e || !n) return T5G_EINVAL;
    *n = e->xl_launches;
    return T5G_OK;
}

extern "C" int t5g_engine_set_fused(t5g_engine* e, int32_t enable) {
    if (!e) return T5G_EINVAL;
    if (e->fused_mlp != (enable != 0)) {
        e->fused_mlp = enable != 0;
        drop_graphs(e);   // captured launches follow the flag
    }
    return T5G_OK;
}

extern "C" int t5g_write_state(t5g_engine* e, const t5g_sampler_state* s, int32_t row, int32_t slot, int32_t token,
                               void* stream) {
    if (!e || !s || row < 0 || row >= e->c.max_batch || slot < 0 || slot >= e->c.max_gen) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    static thread_local t5g_sampler_state hs;
    static thread_local int32_t hv[3];
    hs = *s;
    HIPCHK(hipMemcpyAsync(e->state + row, &hs, sizeof(SamplerState), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->out_tokens + (size_t)row * e->c.max_gen + slot, &token, sizeof(int),
                          hipMemcpyHostToDevice, st));
    if (!s->done) {
        hv[0] = s->current_length;
        hv[1] = token;
        float p = s->next_pos;
        HIPCHK(hipMemcpyAsync(e->kv_len + row, &hv[0], sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->next_token + row, &hv[1], sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->next_pos + row, &p, sizeof(float), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return T5G_OK;
}

extern "C" int t5g_step_only(t5g_engine* e, void* stream) {
    if (!e || e->B <= 0) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    // replayed from a graph: the step reads its tokens / positions / lengths from device
    // memory, so one capture per batch size serves every step (~250 launches in parity mode)
    if (!e->gexec_fwd || e->graph_fwd_B != e->B) {
        if (e->gexec_fwd) hipGraphExecDestroy(e->gexec_fwd);
        if (e->graph_fwd) hipGraphDestroy(e->graph_fwd);
        e->gexec_fwd = nullptr;
        e->graph_fwd = nullptr;
        const int rc = capture(e, [&](hipStream_t cs) { return decode_forward(e, cs); }, &e->graph_fwd, &e->gexec_fwd);
        if (rc) return rc;   // the fast path's graphs stay
        e->graph_fwd_B = e->B;
    }
    HIPCHK(hipGraphLaunch(e->gexec_fwd, st));
    return T5G_OK;
}

extern "C" int t5g_read_flags(t5g_engine* e, int32_t* out, int32_t B, void* stream) {
    if (!e || !out || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(out, e->flags, B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return T5G_OK;
}

extern "C" int t5g_read_step(t5g_engine* e, t5g_sampler_state* state_out, int32_t* flags_out, int32_t B,
                             void* stream) {
    if (!e || !state_out || !flags_out || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(state_out, e->state, B * sizeof(SamplerState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(flags_out, e->flags, B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return T5G_OK;
}

extern "C" void* t5g_logits_ptr(t5g_engine* e, int32_t* ld) {
    if (!e) return nullptr;
    if (ld) *ld = e->logits_ld;
    return e->logits;
}

extern "C" int t5g_engine_set_rope_exc(t5g_engine* e, const uint32_t* tab, int32_t n) {
    if (!e || n < 0 || (n > 0 && !tab)) return T5G_EINVAL;
    if (e->trig_exc) {
        (void)hipFree(e->trig_exc);
        e->trig_exc = nullptr;
    }
    e->n_trig_exc = 0;
    if (n == 0) return T5G_OK;
    HIPCHK(hipMalloc(&e->trig_exc, (size_t)n * 8));
    HIPCHK(hipMemcpy(e->trig_exc, tab, (size_t)n * 8, hipMemcpyHostToDevice));
    e->n_trig_exc = n;
    return T5G_OK;
}

extern "C" void* t5g_engine_cache_ptr(t5g_engine* e, int32_t layer, int32_t which, int64_t* head_stride,
                                      int64_t* row_stride) {
    if (!e || layer < 0 || layer >= e->c.n_dec_layers || which < 0 || which > 3) return nullptr;
    const int cap = which < 2 ? e->c.max_audio : e->c.max_text;
    if (head_stride) *head_stride = (int64_t)cap * e->c.head_dim;
    if (row_stride) *row_stride = (int64_t)cap * e->c.head_dim * e->c.n_kv_heads;
    return which == 0 ? e->sk[layer] : which == 1 ? e->sv[layer] : which == 2 ? e->ck[layer] : e->cv[layer];
}

extern "C" int t5g_copy_logits(t5g_engine* e, void* dst, int32_t B, void* stream) {
    if (!e || !dst || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    HIPCHK(hipMemcpyAsync(dst, e->logits, (size_t)B * e->logits_ld * sizeof(bf16_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return T5G_OK;
}

extern "C" int t5g_sample_only(t5g_engine* e, int32_t B, const void* logits, int32_t ld, void* stream) {
    if (!e || B <= 0 || B > e->c.max_batch) return T5G_EINVAL;
    RC(sample(sampler_args(e, (const bf16_t*)logits, ld, B), (hipStream_t)stream));
    return T5G_OK;
}

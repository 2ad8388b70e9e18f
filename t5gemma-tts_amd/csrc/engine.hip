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
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <vector>

#include "../../include/t5gtts.h"
#include "ref_ksplit.h"
#include "t5g_kernels.h"

using namespace t5g;

#define HIPCHK(x)                                  \
    do {                                           \
        if ((x) != hipSuccess) return T5G_EHIP;    \
    } while (0)
#define RC(x)                       \
    do {                            \
        int _rc = (x);              \
        if (_rc) return _rc == -1 ? T5G_EINVAL : (_rc == -3 ? T5G_EUNSUPPORTED : T5G_EHIP); \
    } while (0)

constexpr int GRAPH_STEPS = 8;   // decode iterations per multi-step graph

static inline int ng_pad(int N) { return ((N + 15) / 16 + 3) / 4 * 4; }

struct t5g_engine {
    t5g_config c;
    t5g_weights w;
    std::vector<t5g_layer_weights> enc, dec;
    int q_dim, kv_dim, qkv_dim, V, Vpad;
    int max_tok;  // packed token capacity for encode / prefill
    // arena
    std::vector<void*> allocs;
    int64_t bytes = 0;
    // packed-token activations (encode / prefill)
    bf16_t *h, *xn, *qkv, *q, *att, *act, *tmp, *mem;
    float* part;          // split-K slabs (max over uses)
    int64_t part_elems;
    bf16_t *enc_k, *enc_v;                 // encoder self K/V [B][Hkv][max_text][D]
    std::vector<bf16_t*> ck, cv, sk, sv;   // per decoder layer cross / self caches
    int* enc_len;                          // [B] text lengths
    // decode (rows = max_batch)
    bf16_t *dh, *dxn, *dq, *datt, *dact, *dhh, *logits;
    int logits_ld;
    // sampler
    SamplerRow* rows;
    SamplerState* state;
    int* topk_list;
    int* silence;
    int* out_tokens;
    int* kv_len;
    float* next_pos;
    int* next_token;
    int* flags;
    int* last_rows;
    float* rope_tab;    // [max_batch][D] per-row cos|sin of the decode step's PM position
    // multi-block sampler scratch (sampler.hip fast path)
    float* fs_val;
    int* fs_idx;
    int* fs_cnt;
    float* fs_amv;
    int* fs_ami;
    unsigned* fs_ticket;
    int* fs_slow;
    bool fast_sampler = true;   // false: single-block sampler only (t5g_engine_set_sampler_path)
    // decode MLP half as one persistent launch (fused.hip; t5g_engine_set_fused)
    bool fused_mlp = true;
    float* part2 = nullptr;     // the fused block's in-launch slabs: cross-q [2][B][q_dim] | cross-o [4][B][d] | down [8][B][d] | self o [4][B][d]
    bf16_t* datt2 = nullptr;    // the fused block's cross-attention output [B][q_dim]
    unsigned* fsync = nullptr;  // timeout line + one fused.hip counter set per decoder layer + one xlayer.hip
                                // set per decoder layer (zeroed at creation / after a timeout)
    // decode split-K factors (measured on MI355X): qkv 2, o / cross-q /
    // cross-o 4, down 8 k-slices; gate/up on the one-block-per-CU GEMV
    static constexpr int s_qkv = 2, s_o = 4, s_down = 8;
    float* asbuf = nullptr;   // decode attention scores of rows > 64 keys [B][Hq][max(max_audio, max_text)]
    float* ambuf = nullptr;   // decode attention chunk maxima [B][Hkv][nsplit][G]
    // flash-form decode attention (fast path, t5g_engine_set_attn_flash): chunk partials,
    // chunk (max, sum), one arrival ticket per (row, kv head) -- zeroed here, left zero
    bool attn_flash = true;
    // the flash decode self-attention as stage S of the persistent layer launch (fast path,
    // t5g_engine_set_attn_in_block): no attention launch of its own between the layers
    int attn_in_block = 2;   // 0 own launch, 1 stage S in front of O1, 2 at the end of the previous launch
    // the largest batch the whole-layer launch takes (t5g_engine_set_block_max_rows): 16 (one
    // MFMA tile) or 32 (two tiles, fused_rows32.hip); larger batches run the per-op launches
    // with the MLP-half launch
    int block_max_rows = 16;
    int64_t blk_launches = 0;   // whole-layer launches issued (t5g_engine_block_launches)
    int64_t s_launches = 0;   // persistent layer launches run with stage S (tests)
    int s_mode_used = 0;      // the last decode pass's stage-S placement: 2 tail, 1 front, 0 none
    float* afpart = nullptr;    // [B][Hkv][nsplit][G][D]
    float* afstat = nullptr;    // [B][Hkv][nsplit][G][2]
    unsigned* aftick = nullptr; // [B][Hkv]
    int B = 0;            // rows of the current call
    int text_max = 0;     // longest text of the current call (host hint; 0: max_text)
    int audio_max = 0;    // key bound of the current call's rows (host hint; 0: max_audio)
    const bf16_t* noise = nullptr;
    int noise_steps = 0;
    const uint32_t* noise_mt = nullptr;   // parity mode: raw MT19937 outputs [B][noise_mt_steps][2 V] (noise.hip)
    int noise_mt_steps = 0;
    // graphs of one and of GRAPH_STEPS decode iterations (a replay boundary costs
    // ~10 us; back-to-back iterations inside one graph only the kernel boundaries)
    hipGraph_t graph = nullptr, graph_n = nullptr;
    hipGraphExec_t gexec = nullptr, gexec_n = nullptr;
    int graph_B = -1;
    // graph of one decoder step + head without the sampler (t5g_step_only: parity mode)
    hipGraph_t graph_fwd = nullptr;
    hipGraphExec_t gexec_fwd = nullptr;
    int graph_fwd_B = -1;
    hipStream_t graph_stream = nullptr;
    hipStream_t cap_stream = nullptr;
    // parity mode (t5g_engine_set_exact): every sum in the reference host's CPU order
    bool exact = false;
    int exact_threads = REF_KSPLIT_THREADS;
    uint16_t* ksplit_dev = nullptr;     // ref_ksplit.h tables [REF_KSPLIT_NSHAPES][REF_KSPLIT_MAX_M]
    uint16_t* gelu_lut_dev = nullptr;   // [65536] bf16 -> bf16 nn.GELU() of the reference host
    uint16_t* tanh_lut_dev = nullptr;   // [65536] bf16 -> bf16 torch.tanh of the reference host (eager)
    // parity mode's Linears on the f32 MFMA (xmm.hip): E16 copies of the packed weights
    // (made once, at the first t5g_engine_set_exact) and X16 activation buffers
    struct XLayer {
        bf16_t *qkv, *o, *gate_up, *down, *cross_q, *cross_kv, *cross_o;
    };
    std::vector<XLayer> enc_x, dec_x;
    bf16_t *head1_x = nullptr, *head2_x = nullptr;
    bf16_t *xn16 = nullptr, *att16 = nullptr, *act16 = nullptr, *mem16 = nullptr;   // packed tokens
    bf16_t *dxn16 = nullptr, *datt16 = nullptr, *dact16 = nullptr, *dhh16 = nullptr;   // decode rows
    float* dpart = nullptr;   // decode down projection: fp32 K-part values [4][B16][hidden]
    uint32_t* trig_exc = nullptr;   // parity mode: RoPE cos / sin exceptions (t5g_engine_set_rope_exc)
    int n_trig_exc = 0;
    bool xmm_ready = false;
    // the timing hooks (t5g_time_*) re-run launches on the live decode state (h, the KV slot
    // of the last step, the attention scratch): t5g_decode refuses to continue from it until a
    // t5g_sampler_setup (after a fresh prefill) starts a new call
    bool decode_state_invalid = false;
    int64_t xl_launches = 0;   // xlayer.hip launches issued (captured ones counted once, at capture)
};

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
static int gemm(const bf16_t* X, int ldx, int M, const void* W, int N, int K, int splits, const void* bias,
                void* Y, int ldy, int epi, hipStream_t st, bool prefill = false, bool pf_reg = false) {
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

static NormArgs norm_args(int M, int d, float eps) {
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
static int xlin16(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, const void* bias,
                  void* Y, int ldy, bf16_t* Y16, int epi, const int* tok_row, const int* row_len, int nref_a,
                  int nref_b, int nsplit_col, hipStream_t st) {
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
static int xlin16_dec_parts(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, void* Y,
                            int ldy, const int* tok_row, int* nparts, hipStream_t st) {
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
static bool xlayer_usable(const t5g_engine* e, int M) {
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

static XLayerArgs xlayer_args(t5g_engine* e, int M, int l) {
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

// One decoder pass over `M` tokens. Packed mode (tok_row != null): prefill;
// decode mode: M = B rows, positions/slots/tokens from the sampler buffers.
static DecGemmArgs dec_args(int M, const void* W, int N, int K, void* Y, int ldy, int nw);

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
static FusedMlpArgs fused_args(t5g_engine* e, int M, int l) {
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

// the same launch with the cross-attention chain in front (fused.hip fused_block_kernel):
// o-proj slabs in e->part -> ... -> down slabs in e->part
static FusedMlpArgs fused_block_args(t5g_engine* e, int M, int l) {
    const t5g_config& c = e->c;
    const t5g_layer_weights& L = e->dec[l];
    FusedMlpArgs fa = fused_args(e, M, l);
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
    return fa;
}

// stage S in front (fast path): the layer's flash decode self-attention inside the launch,
// with decode_attention's arguments (the cache, the call's chunk grid, the q|k|v slabs);
// false when the launch is not built for them (the attention then runs as its own launch)
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
static bool fused_block_tail(t5g_engine* e, int M, int l, FusedMlpArgs& fa) {
    const t5g_config& c = e->c;
    fa.Wo1 = nullptr;   // the o-projection of this layer ran at the end of the previous launch
    fa.o_slabs = l == 0 ? e->part : fa.o1slab;
    if (l == c.n_dec_layers - 1) return fused_mlp_check(fa) == 0;
    fused_s_fields(e, l + 1, fa);
    fa.self_tail = 1;
    fa.Wo1n = (const bf16_t*)e->dec[l + 1].o;
    fa.o1n = fa.o1slab;
    fa.att_self = e->datt;
    (void)M;
    return fused_mlp_check(fa) == 0;
}

static bool fused_block_self(t5g_engine* e, int M, int l, FusedMlpArgs& fa) {
    const t5g_config& c = e->c;
    // mode 1, or mode 2 on a call the tail does not take (2 slots per worker): S in front
    if (e->attn_in_block < 1 || !e->attn_flash || !fa.Wo1) return false;
    fa.self_attn = 1;
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
    if (fused_mlp_check(fa) != 0) {
        fa.self_attn = 0;
        return false;
    }
    (void)M;
    return true;
}

static int decoder_pass(t5g_engine* e, int M, const int* ids, const int* tok_row, const int* tok_t, const float* pos,
                        bool decode, hipStream_t st) {
    const t5g_config& c = e->c;
    const int d = c.hidden, f = c.intermediate, D = c.head_dim;
    bf16_t* h = decode ? e->dh : e->h;
    bf16_t* xn = decode ? e->dxn : e->xn;
    bf16_t* q = decode ? e->dq : e->q;
    bf16_t* att = decode ? e->datt : e->att;
    bf16_t* act = decode ? e->dact : e->act;
    bf16_t* tmp = e->tmp;
    // eager checkpoints (softcap > 0) take the same decode launches: the attention kernels
    // apply the tanh softcap in the score (common.h fast_score)
    // split-K factors (decode: spread the weight streams over >= 512 blocks)
    const int s_qkv = decode ? e->s_qkv : 1, s_o = decode ? e->s_o : 1, s_down = decode ? e->s_down : 1;
    // one cos/sin table per step: every layer's q/k rotation uses the same positions
    // (written by layer 0's embedding-norm launch below)
    const float* tab = decode ? e->rope_tab : nullptr;
    // norm after a Linear: h = h + RMSNorm_post(delta), xn = RMSNorm_pre(h)
    auto resid = [&](int splits, const void* post_w, const void* pre_w) -> int {
        NormArgs n = norm_args(M, d, c.rms_eps);
        if (splits > 1) {
            n.part = e->part;
            n.nsplit = splits;
            n.ldp = d;
        } else {
            n.delta = tmp;
        }
        n.post_w = (const bf16_t*)post_w;
        n.resid = h;
        n.pre_w = (const bf16_t*)pre_w;
        n.resid_out = h;
        n.normed_out = xn;
        return resid_norm(n, st);
    };
    // attention output projection into the norm's fp32 slabs: at the 2b-2b width (K = 2048,
    // 4 slices of 16 k-steps) on the register-resident-X GEMV for every batch size up to 32,
    // so a row's sums never depend on the batch (tools/probe_proj_rx.py: 4.13 vs 4.23 us at
    // 8 rows, 5.2 vs 6.8 at 32)
    auto out_proj = [&](const bf16_t* x, const void* W) -> int {
        if (decode && M <= 32 && d == 2304 && e->q_dim == 2048 && s_o == 4) {
            DecGemmArgs g = dec_args(M, W, d, e->q_dim, e->part, d, 8);
            g.X = x;
            g.ldx = e->q_dim;
            g.splits = s_o;
            g.layout_rx = 1;
            // -1: the register-X GEMV's per-block LDS does not fit this device's CU count
            // (e.g. a CPX partition): the tiled split-K GEMM below
            const int rc = gemv_dec(g, EPI_F32, st);
            if (rc != -1) return rc;
        }
        return gemm(x, e->q_dim, M, W, d, e->q_dim, s_o, nullptr, s_o > 1 ? (void*)e->part : (void*)tmp, d,
                    s_o > 1 ? EPI_F32 : EPI_BF16, st, !decode);
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
        r.rope_tab = tab;
        r.Qout = q;
        r.ldq = e->q_dim;
        return r;
    };
    bool qkv_done = false;   // the previous layer's fused block projected this layer's q|k|v
    // stage S at the end of the launches (attn_in_block 2): every layer's launch must take it
    bool tail = false;
    if (decode && e->attn_in_block == 2 && e->attn_flash && e->fused_mlp && M <= e->block_max_rows && d == 2304 && f == 9216 &&
        s_o == 4 && s_down == 8 && s_qkv == 2 && e->q_dim == 2048 && c.n_dec_layers >= 2) {
        tail = true;
        for (int l = 0; l < c.n_dec_layers && tail; ++l) {
            FusedMlpArgs fa = fused_block_args(e, M, l);
            tail = fused_block_tail(e, M, l, fa);
        }
    }
    if (decode) e->s_mode_used = tail ? 2 : 0;
    for (int l = 0; l < c.n_dec_layers; ++l) {
        const t5g_layer_weights& L = e->dec[l];
        if (l == 0) {
            NormArgs n = norm_args(M, d, c.rms_eps);
            n.ids = ids;
            n.table = (const bf16_t*)e->w.audio_embed;
            n.n_table = c.n_audio_tokens;
            n.scale = c.normalizer;
            n.pre_w = (const bf16_t*)L.norms[0];
            n.resid_out = h;
            n.normed_out = xn;
            if (decode) {   // and the step's RoPE table, in the same launch
                n.rope_pos = pos;
                n.rope_inv_freq = e->w.inv_freq;
                n.rope_tab = e->rope_tab;
                n.rope_D = D;
            }
            RC(resid_norm(n, st));
        }
        // --- self attention
        const int win = c.dec_sliding[l] ? c.sliding_window : 0;
        if (decode) {
            // q|k|v as fp32 split-K slabs; q rotated, k rotated + appended inside attention.
            // At the 2b-2b width: the 12-wave register-X GEMV over 2 k-slices (the fused
            // block's QKV stage, which produced them already when qkv_done)
            if (!qkv_done) {
                int rcq = -1;
                if (M <= 32 && d == 2304 && s_qkv == 2) {
                    DecGemmArgs g = dec_args(M, L.qkv, e->qkv_dim, d, e->part, e->qkv_dim, 12);
                    g.X = xn;
                    g.ldx = d;
                    g.splits = 2;
                    g.layout_rx = 1;
                    rcq = gemv_dec(g, EPI_F32, st);
                    if (rcq != 0 && rcq != -1) RC(rcq);
                }
                if (rcq != 0) RC(gemm(xn, d, M, L.qkv, e->qkv_dim, d, s_qkv, nullptr, e->part, e->qkv_dim, EPI_F32, st));
            }
            qkv_done = false;
            if (tail) {
                // layer 0's attention and o-projection as their own launches (the step's
                // prologue), then every layer's launch runs the next layer's attention and
                // o-projection at its end (bitwise equal to the launches below)
                if (l == 0) {
                    RC(decode_attention(e, M, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1, win, 0, true, pos, tab,
                                        s_qkv, e->qkv_dim, st));
                    RC(out_proj(att, L.o));
                }
                FusedMlpArgs fa = fused_block_args(e, M, l);
                if (!fused_block_tail(e, M, l, fa)) return T5G_EUNSUPPORTED;   // checked for every layer above
                RC(fused_mlp(fa, st));
                ++e->blk_launches;
                if (l != c.n_dec_layers - 1) ++e->s_launches;
                qkv_done = true;
                continue;
            }
            // the persistent layer launch with the attention as its stage S (bitwise equal to
            // the flash launch below followed by the same launch without S)
            if (e->fused_mlp && M <= e->block_max_rows && d == 2304 && f == 9216 && s_o == 4 && s_down == 8 && s_qkv == 2 &&
                e->q_dim == 2048 && c.n_dec_layers >= 2) {
                FusedMlpArgs fa = fused_block_args(e, M, l);
                if (fused_mlp_check(fa) == 0 && fused_block_self(e, M, l, fa)) {
                    RC(fused_mlp(fa, st));
                    ++e->blk_launches;
                    ++e->s_launches;
                    e->s_mode_used = 1;
                    qkv_done = l != c.n_dec_layers - 1;
                    continue;
                }
            }
            RC(decode_attention(e, M, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1, win, 0, true, pos, tab, s_qkv,
                                e->qkv_dim, st));
        } else {
            RC(gemm(xn, d, M, L.qkv, e->qkv_dim, d, 1, nullptr, e->qkv, e->qkv_dim, EPI_BF16, st, !decode));
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
            RC(attn_packed(e, M, q, tok_row, tok_t, e->sk[l], e->sv[l], c.max_audio, e->kv_len, 1, win, att, st));
        }
        const bool last = l == c.n_dec_layers - 1;
        // the rest of the layer (o-projection, cross attention, MLP half, the last norm and
        // the next layer's q|k|v) as one persistent launch (fused.hip fused_block_kernel;
        // bitwise equal to the launches below)
        if (decode && e->fused_mlp && M <= e->block_max_rows && d == 2304 && f == 9216 && s_o == 4 && s_down == 8 &&
            e->q_dim == 2048 && c.n_dec_layers >= 2) {
            const FusedMlpArgs fa = fused_block_args(e, M, l);
            if (fused_mlp_check(fa) == 0) {
                RC(fused_mlp(fa, st));
                ++e->blk_launches;
                qkv_done = !last;
                continue;
            }
        }
        RC(out_proj(att, L.o));
        RC(resid(s_o, L.norms[1], L.norms[2]));
        // --- PM cross attention (q rotated by the decoder progress, :149-165)
        if (decode) {
            // cross-q: at the 2b-2b width the register-X GEMV over 2 k-slices of 36 k-steps,
            // 12 waves (the fused block's Q stage), so a row's sums never depend on the batch
            int s_q = s_o, rcq = -1;
            if (M <= 32 && d == 2304 && e->q_dim == 2048) {
                DecGemmArgs g = dec_args(M, L.cross_q, e->q_dim, d, e->part, e->q_dim, 12);
                g.X = xn;
                g.ldx = d;
                g.splits = 2;
                g.layout_rx = 1;
                rcq = gemv_dec(g, EPI_F32, st);
                if (rcq == 0) s_q = 2;
                else if (rcq != -1) RC(rcq);
            }
            if (rcq != 0) RC(gemm(xn, d, M, L.cross_q, e->q_dim, d, s_o, nullptr, e->part, e->q_dim, EPI_F32, st));
            RC(decode_attention(e, M, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, 0, false, pos, tab, s_q,
                                e->q_dim, st));
        } else {
            RC(gemm(xn, d, M, L.cross_q, e->q_dim, d, 1, nullptr, q, e->q_dim, EPI_BF16, st, !decode));
            RopeArgs r = rope_args();
            r.X = q;
            r.ldx = e->q_dim;
            r.nq = c.n_heads;
            r.rope_q = 1;
            RC(rope_store(r, st));
            RC(attn_packed(e, M, q, tok_row, tok_t, e->ck[l], e->cv[l], c.max_text, e->enc_len, 0, 0, att, st));
        }
        RC(out_proj(att, L.cross_o));
        // --- norm + GeGLU MLP: at the 2b-2b width, decode rows <= 32, one persistent launch
        // (fused.hip; bitwise equal to the three launches below)
        if (decode && e->fused_mlp && M <= 32 && d == 2304 && f == 9216 && s_o == 4 && s_down == 8 &&
            c.n_dec_layers >= 2) {
            const int rc = fused_mlp(fused_args(e, M, l), st);
            if (rc == 0) {
                RC(resid(s_down, L.norms[5], last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]));
                continue;
            }
            if (rc != -1) RC(rc);   // -1: a shape / device the launch is not built for
        }
        RC(resid(s_o, L.norms[3], L.norms[4]));
        // --- GeGLU MLP (decode: the one-block-per-CU GEMV; register-resident X at the
        // 2b-2b width, up to 32 rows)
        if (decode && (M <= 16 || (M <= 32 && d == 2304))) {
            DecGemmArgs g = dec_args(M, L.gate_up, 2 * f, d, act, f, d == 2304 ? 12 : 8);
            g.X = xn;
            g.ldx = d;
            // register-X at 2b-2b width: every unit's weights requested up front (18.84 ->
            // 18.39 us at 8 rows, 24.2 -> 23.9 at 32, bitwise equal: tools/probe_rx_all.py)
            g.un = d == 2304 ? -1 : 8;
            g.layout_rx = d == 2304;
            const int rc = gemv_dec(g, EPI_GEGLU, st);
            if (rc == -1) RC(gemm(xn, d, M, L.gate_up, 2 * f, d, 1, nullptr, act, f, EPI_GEGLU, st, !decode));
            else RC(rc);
        } else {
            RC(gemm(xn, d, M, L.gate_up, 2 * f, d, 1, nullptr, act, f, EPI_GEGLU, st, !decode));
        }
        if (decode && M <= 32 && d == 2304 && f == 9216 && s_down == 8) {
            // down: register-resident X over 36-k-step slices, 32 blocks per slice
            // (tools/probe_down_rx.py: 11.2 vs 16.3 us at 32 rows, 9.0 vs 9.4 at 8)
            DecGemmArgs g = dec_args(M, L.down, d, f, e->part, d, 12);
            g.X = act;
            g.ldx = f;
            g.splits = s_down;
            g.layout_rx = 1;
            const int rc = gemv_dec(g, EPI_F32, st);
            if (rc == -1) RC(gemm(act, f, M, L.down, d, f, s_down, nullptr, e->part, d, EPI_F32, st, false));
            else RC(rc);
        } else {
            RC(gemm(act, f, M, L.down, d, f, s_down, nullptr, s_down > 1 ? (void*)e->part : (void*)tmp, d,
                    s_down > 1 ? EPI_F32 : EPI_BF16, st, !decode));
        }
        RC(resid(s_down, L.norms[5], last ? e->w.dec_final_norm : e->dec[l + 1].norms[0]));
    }
    return T5G_OK;
}

static DecGemmArgs dec_args(int M, const void* W, int N, int K, void* Y, int ldy, int nw) {
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

// one decoder step + predict head for the e->B rows fed by the sampler buffers
static int head(t5g_engine* e, const bf16_t* xn_rows, int B, hipStream_t st);
static int head_exact(t5g_engine* e, const bf16_t* xn_rows16, int B, hipStream_t st);
static int decode_forward(t5g_engine* e, hipStream_t st) {
    if (e->exact) {
        RC(decoder_pass_exact(e, e->B, e->next_token, nullptr, nullptr, e->next_pos, true, st));
        return head_exact(e, e->dxn16, e->B, st);
    }
    int rc = decoder_pass(e, e->B, e->next_token, nullptr, nullptr, e->next_pos, true, st);
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
        DecGemmArgs g = dec_args(B, e->w.head2, e->V, d, e->logits, e->logits_ld, 4);
        g.X = e->dhh;
        g.ldx = d;
        g.un = 8;
        g.layout_rx = 1;
        g.bias = (const bf16_t*)e->w.head2_bias;
        const int rc = gemv_dec(g, EPI_BIAS_BF16, st);
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
                      : decoder_pass(e, ntok, ids, tok_row, tok_t, pos, false, st);
    if (rc) return rc;
    // the last decoder_pass norm wrote final-normed hidden of every token into xn;
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
        if (!e->cap_stream) HIPCHK(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        for (int which = 0; which < 2; ++which) {
            HIPCHK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
            int rc = T5G_OK;
            for (int i = 0; i < (which ? GRAPH_STEPS : 1) && !rc; ++i) rc = decode_iter(e, e->cap_stream);
            hipGraph_t g = nullptr;
            hipError_t ec = hipStreamEndCapture(e->cap_stream, &g);
            if (rc || ec != hipSuccess) {
                if (g) hipGraphDestroy(g);
                drop_graphs(e);
                return rc ? rc : T5G_EHIP;
            }
            hipGraphExec_t x = nullptr;
            if (hipGraphInstantiate(&x, g, nullptr, nullptr, 0) != hipSuccess) {
                hipGraphDestroy(g);
                drop_graphs(e);
                return T5G_EHIP;
            }
            (which ? e->graph_n : e->graph) = g;
            (which ? e->gexec_n : e->gexec) = x;
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
static int check_handoff(t5g_engine* e, hipStream_t st) {
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
        if (!e->cap_stream) HIPCHK(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
        HIPCHK(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
        const int rc = decode_forward(e, e->cap_stream);
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
        e->graph_fwd = g;
        e->gexec_fwd = x;
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

extern "C" int t5g_sort_emu_wave(int32_t n, int32_t S, int32_t* pos_dev, float* val_dev, int32_t* tag_dev,
                                 int32_t* fail_dev, void* stream) {
    RC(sort_emu_wave(n, S, pos_dev, val_dev, tag_dev, fail_dev, (hipStream_t)stream));
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
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const bool pf = (epi & T5G_GEMM_PREFILL) != 0, pf_reg = (epi & T5G_GEMM_PREFILL_REG) != 0;
    epi &= 0xff;
    RC(gemm((const bf16_t*)X, ldx, M, Wp_list[0], N, K, splits, nullptr, Y, ldy, epi, st, pf, pf_reg));  // warm
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i)
        RC(gemm((const bf16_t*)X, ldx, M, Wp_list[i % n_w], N, K, splits, nullptr, Y, ldy, epi, st, pf, pf_reg));
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return T5G_OK;
}

extern "C" int t5g_time_decode_step(t5g_engine* e, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || e->B <= 0) return T5G_EINVAL;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) {
        int rc = decode_forward(e, st);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return check_handoff(e, st);
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
    RC(layer(0));   // untimed: the first launch's one-time setup
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) RC(layer(i % c.n_dec_layers));
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return T5G_OK;
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
    for (int l = 0; l < L; ++l) {
        const int rc = xlayer_launch(xlayer_args(e, B, l), st);
        if (rc) return rc == -1 ? T5G_EUNSUPPORTED : T5G_EHIP;
    }
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    int rc = 0;
    // diagnostic T5G_TIME_SHARE: "chain" -- every launch reads layer 1's o / cross q / cross o /
    // q|k|v weights and cross K / V (its G / D weights rotate); "gd" -- layer 1's gate/up and
    // down (the rest rotates): which bytes' cache residency the launch is sensitive to
    const char* share_s = getenv("T5G_TIME_SHARE");
    const int share = !share_s ? 0 : !strcmp(share_s, "chain") ? 1 : !strcmp(share_s, "gd") ? 2 : 0;
    const XLayerArgs a1 = xlayer_args(e, B, 1);
    for (int i = 0; i < n && !rc; ++i) {
        XLayerArgs a = xlayer_args(e, B, i % L);
        if (share == 1 && a.Wqkv) {
            a.Wo = a1.Wo, a.Wq = a1.Wq, a.Wco = a1.Wco, a.Wqkv = a1.Wqkv, a.ck = a1.ck, a.cv = a1.cv;
        } else if (share == 2) {
            a.Wgu = a1.Wgu, a.Wd = a1.Wd;
        }
        rc = xlayer_launch(a, st);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) return rc == -1 ? T5G_EUNSUPPORTED : T5G_EHIP;
    *avg_us = ms * 1000.f / (float)n;
    return check_handoff(e, st);
}

// hipEvent-timed fused decode-MLP launches (bench.py roofline leg): layers rotated, so every
// launch streams its weights from HBM (2.2 GB of gate/up + down > the 256 MiB Infinity Cache)
extern "C" int t5g_time_decode_mlp(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us) {
    if (!e || iters <= 0 || !avg_us || B <= 0 || B > e->c.max_batch || e->c.n_dec_layers < 2) return T5G_EINVAL;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const int L = e->c.n_dec_layers;
    // whole rotations over the layers, as a decode step runs them: layer l's launch finds
    // its counter set zeroed by layer l - 1's (the last launch before this call was a step's
    // last layer, which zeroed layer 0's set); one untimed rotation first
    const int n = (iters + L - 1) / L * L;
    // the launch decoder_pass runs at B rows: the cross-attention chain + MLP block up to
    // 16 rows when the device supports it, the MLP half alone otherwise
    const bool block = B <= 16 && fused_mlp_check(fused_block_args(e, B, 0)) == 0;
    auto args = [&](int l) { return block ? fused_block_args(e, B, l) : fused_args(e, B, l); };
    int rc = T5G_OK;
    for (int l = 0; l < L && !rc; ++l) rc = fused_mlp(args(l), st);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < n && !rc; ++i) rc = fused_mlp(args(i % L), st);
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) return rc == -1 ? T5G_EUNSUPPORTED : T5G_EHIP;
    *avg_us = ms * 1000.f / (float)n;
    return check_handoff(e, st);   // a timed launch that gave up would report a false rate
}

// hipEvent-timed persistent layer launches WITH the self-attention stage S, as the fast
// decode step runs them (bench.py roofline leg): whole rotations over the layers at the
// cache lengths the last call left (each launch re-appends its rows' last key and value, the
// values the slabs in e->part give). *keys = the keys one launch reads per kv head, summed
// over the rows and averaged over the layers (sliding layers clipped to their window).
extern "C" int t5g_time_decode_layer(t5g_engine* e, int32_t B, int32_t iters, void* stream, float* avg_us,
                                     float* keys) {
    if (!e || iters <= 0 || !avg_us || !keys || B <= 0 || B > e->c.max_batch || e->c.n_dec_layers < 2) return T5G_EINVAL;
    e->decode_state_invalid = true;
    hipStream_t st = (hipStream_t)stream;
    const t5g_config& c = e->c;
    const int L = c.n_dec_layers;
    // attn_in_block 1: launch l runs layer l's attention in front; 2: layer l + 1's at its end
    // (the last launch none; layer 0's is the step's own launch, not timed here)
    // (mode 2 on a call the tail does not take runs S in front, as decoder_pass does)
    // (the hook times the one-tile launch: past 16 rows bench.py prices the MLP-half launch)
    if (B > 16) return T5G_EUNSUPPORTED;
    bool tail = e->attn_in_block == 2;
    FusedMlpArgs fa;
    for (int l = 0; l < L && tail; ++l) {
        fa = fused_block_args(e, B, l);
        tail = fused_block_tail(e, B, l, fa);
    }
    auto args = [&](int l, FusedMlpArgs& fa) {
        fa = fused_block_args(e, B, l);
        if (tail) return fused_block_tail(e, B, l, fa);
        return fused_mlp_check(fa) == 0 && fused_block_self(e, B, l, fa);
    };
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
    // diagnostic T5G_TIME_SHARE (tools/probe_cache_share.py): "chain" -- every launch reads
    // layer 1's cross q / cross o / next q|k|v / next o weights and cross K / V (they then stay
    // in the Infinity Cache; the G / D weights rotate); "gd" -- layer 1's gate/up and down.
    // Each launch keeps its own layer's hand-off counter sets, so the synchronisation is the
    // decode step's (a launch repeating a layer would find its counters un-zeroed)
    const char* share_s = getenv("T5G_TIME_SHARE");
    const int share = !share_s ? 0 : !strcmp(share_s, "chain") ? 1 : !strcmp(share_s, "gd") ? 2 : 0;
    FusedMlpArgs f1;
    if (share && !args(1, f1)) return T5G_EUNSUPPORTED;
    int rc = 0;
    for (int l = 0; l < L && !rc; ++l) rc = args(l, fa) ? fused_mlp(fa, st) : -1;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < n && !rc; ++i) {
        if (!args(i % L, fa)) {
            rc = -1;
            break;
        }
        if (share == 1 && i % L != L - 1) {
            fa.Wq = f1.Wq, fa.Wo = f1.Wo, fa.Wqkv = f1.Wqkv, fa.ck = f1.ck, fa.cv = f1.cv;
            if (fa.Wo1n) fa.Wo1n = f1.Wo1n;
        } else if (share == 2) {
            fa.Wgu = f1.Wgu, fa.Wd = f1.Wd;
        }
        rc = fused_mlp(fa, st);
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    if (rc) return rc == -1 ? T5G_EUNSUPPORTED : T5G_EHIP;
    *avg_us = ms * 1000.f / (float)n;
    return check_handoff(e, st);
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
        g->cap > SDPA_KV_BLOCK * SDPA_MAX_BLOCKS)
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

extern "C" int t5g_time_gemv(const t5g_gemv_args* g, const void* const* Wp_list, int32_t n_w, int32_t iters,
                             void* stream, float* avg_us) {
    if (!g || !Wp_list || n_w <= 0 || iters <= 0 || !avg_us) return T5G_EINVAL;
    std::vector<DecGemmArgs> as((size_t)n_w);
    for (int i = 0; i < n_w; ++i) {
        int rc = gemv_from_abi(g, Wp_list[i], &as[i]);
        if (rc) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    RC(gemv_dec(as[0], g->epi, st));  // warm
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) RC(gemv_dec(as[i % n_w], g->epi, st));
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return T5G_OK;
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
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    a.W = (const bf16_t*)W16_list[0];
    RC(xmm(a, epi, st));
    HIPCHK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; ++i) {
        a.W = (const bf16_t*)W16_list[i % n_w];
        RC(xmm(a, epi, st));
    }
    HIPCHK(hipEventRecord(e1, st));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    *avg_us = ms * 1000.f / iters;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return T5G_OK;
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

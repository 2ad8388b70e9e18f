// The engine's state and the host helpers shared by engine.hip (lifecycle, encode / prefill /
// decode, the decode launch plan) and engine_hooks.hip (the t5g_time_* hooks and the
// stand-alone op wrappers). Internal: the C ABI is include/t5gtts.h.
#pragma once
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
    // the persistent launches (fused.hip) and the register-X GEMV sites of the decode pass are
    // built for exactly these slab counts; no launch condition tests them
    static_assert(s_qkv == 2 && s_o == 4 && s_down == 8, "decode split-K factors the launches assume");
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
    int64_t mlp_launches = 0;   // MLP-half launches issued, either format (t5g_engine_mlp_half_launches)
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
    // FP8 mode (t5g_engine_set_fp8_weights): the P8 images + row scales of the decode step's
    // Linears; the P16 pointers above are then the images of the same W_q. The fast decode
    // step runs its register-X GEMV sites and the head on them: per-op launches at every
    // batch size, unless fp8_block (t5g_engine_set_fp8_block) lets 1-16 rows take the
    // whole-layer launch on the P8 images (fused_p8.hip) and fp8_mlp (t5g_engine_set_fp8_mlp)
    // lets the per-op layers of 1-32 rows run the MLP-half launch on them (fused_mlp_p8.hip)
    bool fp8 = false;
    bool fp8_block = false;
    bool fp8_mlp = false;
    std::vector<t5g_fp8_layer> dec8;
    t5g_fp8_linear head2_8 = {nullptr, nullptr};
};

// ---- the fast decode step's launch plan (engine.hip) ------------------------------------
// How one decode Linear runs on the GEMV (gemv.hip): nw waves over `splits` k-slices, `un`
// units in flight, rx: register-resident X. nw 0: not on the GEMV (the tiled GEMM).
struct GemvSite {
    int nw, splits, un;
    bool rx;
};

// Which launches a fast decode step of M rows issues. decode_plan() is the only place that
// knows the 2b-2b widths and the row limits; the decode pass and the timing hooks consume it.
struct DecodePlan {
    GemvSite qkv, proj, cross_q, gate_up, down;   // the per-op sites (proj: o and cross-o)
    bool mlp_half;   // per-op layers run the MLP half as one launch (-1 from it: the three launches)
    bool block;      // layers may run as the whole-layer launch (per layer: decode_layer_launch)
    bool tail;       // stage S at the end of every layer's launch (every layer's launch takes it)
};
// a layer's launches when stage S is not in the tail, in the order they are tried
enum DecodeLaunch { DL_BLOCK_S, DL_BLOCK, DL_MLP_HALF, DL_PER_OP };

// engine.hip's host helpers that engine_hooks.hip calls too (not exported)
#pragma GCC visibility push(hidden)
// block_rows: the most rows the whole-layer launch takes (a decode step: e->block_max_rows).
// switches false: only the row limit, t5g_engine_set_attn_in_block and the launches' own
// checks decide block / tail -- not t5g_engine_set_fused / _set_attn_flash or the widths
DecodePlan decode_plan(t5g_engine* e, int M, int block_rows, bool switches = true);
// layer l's launch under a plan without the tail (the sliding window differs per layer);
// fa: its arguments (DL_PER_OP: untouched)
DecodeLaunch decode_layer_launch(t5g_engine* e, const DecodePlan& p, int M, int l, FusedMlpArgs& fa);
FusedMlpArgs fused_args(t5g_engine* e, int M, int l);
FusedMlpArgs fused_block_args(t5g_engine* e, int M, int l);
bool fused_block_tail(t5g_engine* e, int l, FusedMlpArgs& fa);
int decode_forward(t5g_engine* e, hipStream_t st);
int check_handoff(t5g_engine* e, hipStream_t st);
int gemm(const bf16_t* X, int ldx, int M, const void* W, int N, int K, int splits, const void* bias, void* Y, int ldy,
         int epi, hipStream_t st, bool prefill = false, bool pf_reg = false);
NormArgs norm_args(int M, int d, float eps);
DecGemmArgs dec_args(int M, const void* W, int N, int K, void* Y, int ldy, int nw);
int xlin16(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, const void* bias, void* Y,
           int ldy, bf16_t* Y16, int epi, const int* tok_row, const int* row_len, int nref_a, int nref_b,
           int nsplit_col, hipStream_t st);
int xlin16_dec_parts(t5g_engine* e, const bf16_t* X16, int M, const bf16_t* W16, int N, int K, void* Y, int ldy,
                     const int* tok_row, int* nparts, hipStream_t st);
bool xlayer_usable(const t5g_engine* e, int M);
XLayerArgs xlayer_args(t5g_engine* e, int M, int l);
#pragma GCC visibility pop

"""Inputs, references and reference-only teeth shared by the kernel-level tests of the fast
path's encoder / prefill kernels: tests/test_gpu_attention_packed.py, test_gpu_rope_store.py
and test_gpu_norm_sources.py launch the kernels; tests/test_kernel_cases_cpu.py asserts, with
no GPU, what those tests rely on before they launch anything -- that a window one key longer or
shorter moves every marked query of the chosen seeds by ten times the bound, that a lost block
rescale moves the windowed block cases as far, that the slab values tell a slab order, and that
the share of RoPE pairs next to a bf16 tie is what the safe-set rule expects. Also the decode
attention call and its fp64 reference (tests/test_gpu_attention.py, test_gpu_attn_chunk_scores.py)
and the order-revealing bf16 generator of the exact-order tests; tests/test_engine_cases_cpu.py
pins what they draw. Last, the fp32 single-op kernels of the codec encoder and the Whisper decoder
(tests/test_gpu_codec_enc_ops.py, test_gpu_whisper_ops.py): the module formulas that serve as
fp64 reference and as fp32 yardstick, the bound built from the two, and the peaked-score inputs.
"""
import functools

import torch

BF16 = torch.bfloat16
SENT = 0x7FC1   # the sentinel's bf16 bit pattern (a NaN payload no kernel produces), as int16


def i16(t):
    return t.contiguous().view(torch.int16)


def sentinel(*shape):
    return torch.full(shape, SENT, dtype=torch.int16).view(BF16)


def hdr_bf16(shape, g):
    """bf16 values over a wide exponent range plus rare huge entries: sums whose bits
    depend on the association order (a plain randn rarely exposes a wrong order)."""
    v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-10, 11, shape, generator=g).float())
    big = torch.rand(shape, generator=g) < 4.0 / shape[-1]
    return torch.where(big, torch.randn(shape, generator=g) * 2.0 ** 14, v).to(BF16)


EPS = 1e-6


def rms_norm(x, w):
    """The model's RMSNorm in fp32, (1 + w) scaling, rounded to bf16 once (tests/test_gpu_gemv.py,
    test_gpu_norm_sources.py)."""
    xf = x.float()
    r = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + EPS)
    return ((xf * r) * (1.0 + w.float())).to(BF16)


# ---------------------------------------------------------------------------
# RoPE trig: where device and host cosf / sinf may round to different bf16 values
def trig_safe(inv_freq, pos):
    """[M][D/2] bool: cos and sin of the fp32 angle both more than 4 fp32 ulps from a bf16 tie
    (fp64 arithmetic; a bf16 step is 2^16 fp32 ulps, so 2^-14 of a step on either side)."""
    ang = (pos[:, None] * inv_freq[None, :]).double()   # the fp32 product, as host and device form it
    safe = torch.ones(ang.shape, dtype=torch.bool)
    for v in (ang.cos().abs(), ang.sin().abs()):
        e = torch.floor(torch.log2(v.clamp(min=2.0 ** -100)))
        frac = torch.remainder(v / torch.exp2(e - 7), 1.0)
        safe &= ((frac - 0.5).abs() > 2.0 ** -14) & (v > 2.0 ** -20)
    return safe


def bf16_step(x, d):
    """The bf16 value d steps (+-1) from x, by its bit pattern (no zeros or infinities here)."""
    b = i16(x).to(torch.int32)
    b = torch.where(x.float() < 0, b - d, b + d) if d else b
    return b.to(torch.int16).view(BF16)


# ---------------------------------------------------------------------------
# split-K slabs
def order_slabs(g, nsplit, M, ld, amp=1.0):
    """fp32 slabs [nsplit][M][ld] whose sum depends on the order: slabs 0 and 1 are +-2^18 x
    noise and cancel exactly when added first; added after the others they cost them their low
    bits (two slabs commute, so only three or more can tell an order)."""
    p = torch.randn(nsplit, M, ld, generator=g) * amp
    if nsplit > 2:
        p[0] *= 2.0 ** 18
        p[1] = -p[0]
    return p.float().contiguous()


def seq_sum(p, order=None):
    """The slabs added one by one in fp32 from 0.f, as the kernels add them."""
    acc = torch.zeros_like(p[0])
    for s in (order if order is not None else range(p.shape[0])):
        acc = acc + p[s]
    return acc


def order_sensitivity(p):
    """Share of the bf16-rounded sums that differ when the slabs are added in reverse."""
    rev = seq_sum(p, range(p.shape[0] - 1, -1, -1))
    return (i16(rev.to(BF16)) != i16(seq_sum(p).to(BF16))).float().mean().item()


# ---------------------------------------------------------------------------
# many-query attention
def attn_inputs(seed, Mq, Hq, Hkv, D, B, cap):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(Mq, Hq, D, generator=g).to(BF16)
    K = torch.randn(B, Hkv, cap, D, generator=g).to(BF16)
    V = torch.randn(B, Hkv, cap, D, generator=g).to(BF16)
    return q, K, V


def key_range(t, L, causal, window):
    """The keys query position t of a row of L keys attends to, [lo, hi)."""
    if causal:
        return (max(0, t - window + 1) if window > 0 else 0), min(t + 1, L)
    if window > 0:
        return max(0, t - window), min(L, t + window + 1)
    return 0, L


def exact_attention(q, K, V, lens, rows, pos, scale, causal, window=0, softcap=0.0):
    """fp64 softmax attention of query i (row rows[i], position pos[i]) over its key range;
    tests/test_gpu_attention.py's _exact with a query position and the bidirectional range.
    softcap > 0: scores softcap * tanh(s / softcap)."""
    Mq, Hq, D = q.shape
    Hkv = K.shape[1]
    out = torch.zeros(Mq, Hq, D, dtype=torch.float64)
    for i in range(Mq):
        b = rows[i]
        lo, hi = key_range(pos[i], lens[b], causal, window)
        if hi <= lo:
            continue
        s = torch.einsum("hgd,hnd->hgn", q[i].double().view(Hkv, Hq // Hkv, D), K[b, :, lo:hi].double()) * scale
        if softcap > 0:
            s = torch.tanh(s / softcap) * softcap
        out[i] = torch.einsum("hgn,hnd->hgd", torch.softmax(s, -1), V[b, :, lo:hi].double()).reshape(Hq, D)
    return out


def attn_bound(exact):
    """The project's bound for the aten-order form (tests/test_gpu_attention.py)."""
    return 2.0 ** -6 * max(1.0, exact.abs().max().item())


# ---------------------------------------------------------------------------
# decode attention (one query per row, at the row's last key): tests/test_gpu_attention.py and
# tests/test_gpu_attn_chunk_scores.py
def decode_exact_attention(q, K, V, lens, scale, window=0):
    """fp64 softmax attention of each row's query (at position lens[b] - 1) over its keys
    [lo, lens[b]), lo = max(0, lens[b] - window) for a sliding window, else 0."""
    B, Hq, D = q.shape
    G = Hq // K.shape[1]
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window > 0 else 0
        for h in range(Hq):
            s = (K[b, h // G, lo:L].double() @ q[b, h].double()) * scale
            out[b, h] = torch.softmax(s, 0) @ V[b, h // G, lo:L].double()
    return out


def decode_attention_call(L, B, lens, Hq=8, Hkv=4, D=256, causal=1, seed=0, flash=False, window=0, cap=None,
                          prepare=None, want_rc=0):
    """One t5g_attention_decode(_flash) call on random bf16 q / K / V (attn_inputs, one query
    per row); returns the output (fp64, [B][Hq][D]) and the host inputs. cap: cache slots per
    (row, kv head), default L; prepare(q, K, V) edits the inputs in place before the upload;
    want_rc != 0: the call must return that status and write nothing (returns None)."""
    import ctypes as C
    from t5gemma_tts_amd import _lib
    lib = _lib.lib()
    cap = L if cap is None else cap
    q, K, V = attn_inputs(seed, B, Hq, Hkv, D, B, cap)
    if prepare is not None:
        prepare(q, K, V)
    dev = "cuda"
    qd, Kd, Vd = q.to(dev), K.to(dev), V.to(dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    out = torch.zeros(B, Hq * D, dtype=BF16, device=dev)
    nb = lib.t5g_attention_decode_work_bytes(B, Hq, Hkv, D, cap)
    assert nb > 0
    work = torch.zeros(nb // 4, dtype=torch.float32, device=dev)   # flash: tickets start at zero
    a = _lib.AttnDecodeArgs(B=B, n_heads=Hq, n_kv_heads=Hkv, head_dim=D, q=qd.data_ptr(), k_cache=Kd.data_ptr(),
                            v_cache=Vd.data_ptr(), cap=cap, kv_len=lens_d.data_ptr(), causal=causal, window=window,
                            scale=D ** -0.5, out=out.data_ptr(), work=work.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fn = lib.t5g_attention_decode_flash if flash else lib.t5g_attention_decode
    if want_rc != 0:
        assert fn(C.byref(a), st) == want_rc
        torch.cuda.synchronize()
        assert int((out != 0).sum().item()) == 0 and int((work != 0).sum().item()) == 0   # nothing launched
        return None
    _lib.check(fn(C.byref(a), st), "attention_decode")
    torch.cuda.synchronize()
    got = out.cpu().view(B, Hq, D).double()
    if flash:   # the tickets are left at zero for the next call
        nt = B * Hkv
        assert int(work[-nt:].view(torch.int32).abs().sum().item()) == 0
    return got, q, K, V


# window edges. A marked query is (row, t, marker key, alt): the marker -- 8 q / |q| for head 0
# of every GQA group (score 8 at |q| ~ sqrt(D): about e^8 times an ordinary key's weight), V = 4
# -- sits on the first key inside the range (it must count; the window one key shorter,
# alt = -1, drops it) or on the first key outside (it must not; alt = +1 takes it in).
def causal_marks(W):
    L0 = 4 * W + 4
    lens = [L0, W, W + 1, W + 9]
    marks = [(0, 2 * W, W, +1), (0, 3 * W + 1, 2 * W + 2, -1), (0, L0 - 1, L0 - 1 - W, +1),
             (1, W - 1, 0, -1),          # t = W - 1: the whole row, key 0 the first inside
             (2, W, 0, +1),              # t = W: key 0 is the first key a window drops
             (3, W, 1, -1), (3, W + 8, 8, +1)]
    plain = [(0, 0), (0, 5), (1, 0), (3, 3)]
    return lens, marks, plain


def bidir_marks(W):
    L0 = 4 * W + 4
    lens = [L0, W + 1, W + 2, 5]
    marks = [(0, W + 2, 2, -1), (0, W + 5, 4, +1),                        # lower edge, mid row
             (0, L0 - W - 3, L0 - 3, -1), (0, L0 - W - 6, L0 - 5, +1),    # upper edge, mid row
             (0, 3, W + 3, -1), (0, 7, W + 8, +1),                        # t < W: range starts at key 0
             (0, L0 - 2, L0 - 2 - W, -1), (0, L0 - 4, L0 - W - 5, +1),    # t + W >= len
             (1, 0, W, -1), (1, W, 0, -1),                                # a row of W + 1 keys: both clipped
             (2, 0, W + 1, +1), (2, W + 1, 0, +1)]
    plain = [(3, 2), (3, 0), (0, 2 * W)]
    return lens, marks, plain


WINDOW_CASES = [(causal, W) for causal in (1, 0) for W in (24, 64)]


@functools.lru_cache(maxsize=None)
def window_case(causal, W):
    """Inputs, exact reference, bound, and the reference-only teeth (asserted here, on the CPU):
    the reference at window W + alt moves every marked query by at least ten times the bound.
    Returns (q, K, V, lens, rows, pos, exact, bound, smallest such move)."""
    lens, marks, plain = causal_marks(W) if causal else bidir_marks(W)
    rows = [m[0] for m in marks] + [p[0] for p in plain]
    pos = [m[1] for m in marks] + [p[1] for p in plain]
    q, K, V = attn_inputs(500 + W + causal, len(rows), 8, 4, 256, len(lens), max(lens) + 3)
    assert len({(b, key) for b, _, key, _ in marks}) == len(marks)   # one key per marker
    for i, (b, t, key, alt) in enumerate(marks):
        assert 0 <= key < lens[b]
        for h in range(4):
            qh = q[i, 2 * h].float()
            K[b, h, key] = (8.0 * qh / qh.norm()).to(BF16)
            V[b, h, key] = 4.0
    for b, L in enumerate(lens):
        K[b, :, L:] = 1e4
        V[b, :, L:] = float("nan")
    scale = 256 ** -0.5
    exact = exact_attention(q, K, V, lens, rows, pos, scale, causal, W)
    bound = attn_bound(exact)
    alt_ref = {d: exact_attention(q, K, V, lens, rows, pos, scale, causal, W + d) for d in (-1, 1)}
    moves = []
    for i, (b, t, key, alt) in enumerate(marks):
        lo, hi = key_range(t, lens[b], causal, W)
        assert (lo <= key < hi) == (alt == -1), (b, t, key)   # inside iff the shorter window drops it
        moves.append((alt_ref[alt][i] - exact[i]).abs().max().item())
        assert moves[-1] >= 10 * bound, (causal, W, b, t, key, moves[-1], bound)
    return q, K, V, lens, rows, pos, exact, bound, min(moves)


# several aten blocks
BLOCK_LEN = 1100
BLOCK_T = [0, 31, 255, 256, 511, 512, 513, 699, 700, 767, 768, 1023, 1024, 1025, 1059, 1060, 1098, 1099]
# windows of the last query (t = 1099). 600: lo = 500, blocks [500, 1012) and [1012, 1100), as
# the kernel counts them from lo; the rescale at key 1012 is block 1's either way of counting
# ((1012 - 500) / 512 = 1012 / 512 = 1). 560: lo = 540, the boundary at key 1052, where an index
# that forgets lo (1052 / 512 = 2) reads another block's factor than (1052 - 540) / 512 = 1.
BLOCK_WINDOWS = [600, 560]


@functools.lru_cache(maxsize=None)
def blocks_case():
    """One row of 1 100 keys (three aten blocks of 512). Every query's head 0 of a GQA group is
    a shared direction plus noise, and keys 700 and 1060 point along it: scores about +8 and +9
    for every query that sees them, so the running max rises in the second block and again in
    the third (under either window: in its first and in its second)."""
    g = torch.Generator().manual_seed(1100)
    q, K, V = attn_inputs(1101, len(BLOCK_T), 8, 4, 256, 1, BLOCK_LEN)
    base = torch.randn(4, 256, generator=g)
    for h in range(4):
        q[:, 2 * h] = (base[h] + 0.5 * q[:, 2 * h].float()).to(BF16)
        K[0, h, 700] = (8.0 * base[h] * 16 / base[h].norm() ** 2).to(BF16)
        K[0, h, 1060] = (9.0 * base[h] * 16 / base[h].norm() ** 2).to(BF16)
    return q, K, V


def planted_scores():
    """Scores of the last query's head 0 against the two planted keys."""
    q, K, V = blocks_case()
    return tuple((q[-1, 0].double() @ K[0, 0, k].double()).item() * 256 ** -0.5 for k in (700, 1060))


@functools.lru_cache(maxsize=None)
def blocks_window_case(window):
    """The last query (t = 1099) under a causal window: (q [1], exact, bound, shift), shift being
    how far the reference moves when the second block's rescale exp(m_1 - m_2) of the first
    block's sums is lost (et = 1) -- also what a rescale taken from another block's slot amounts
    to, up to the factor. Asserted here, from the reference alone: the running max rises by
    more than 0.5 across the boundary and the shift is at least ten times the bound."""
    q, K, V = blocks_case()
    scale, t = 256 ** -0.5, BLOCK_LEN - 1
    qi = q[len(BLOCK_T) - 1:]
    exact = exact_attention(qi, K, V, [BLOCK_LEN], [0], [t], scale, True, window)
    bound = attn_bound(exact)
    lo = t - window + 1
    assert 0 < lo and lo % 512 and 512 < BLOCK_LEN - lo <= 1024 and lo <= 700 < lo + 512 <= 1060
    sc = torch.einsum("hgd,hnd->hgn", qi[0].double().view(4, 2, 256), K[0, :, lo:BLOCK_LEN].double()) * scale
    m1, m2 = sc[:, 0, :512].max(-1).values, sc[:, 0].max(-1).values
    w1 = torch.exp(sc[:, 0, :512] - m1[:, None])          # block one's weights without the rescale
    w2 = torch.exp(sc[:, 0, 512:] - m2[:, None])
    wrong = (torch.einsum("hn,hnd->hd", w1, V[0, :, lo:lo + 512].double()) +
             torch.einsum("hn,hnd->hd", w2, V[0, :, lo + 512:BLOCK_LEN].double())) / (w1.sum(-1) + w2.sum(-1))[:, None]
    shift = (wrong - exact[0].view(4, 2, 256)[:, 0]).abs().max().item()
    assert (m2 > m1 + 0.5).all() and shift >= 10 * bound, (window, m1.tolist(), m2.tolist(), shift, bound)
    return qi, exact, bound, shift


# ---------------------------------------------------------------------------
# fp32 single-op kernels of the codec encoder and the Whisper decoder against fp64
# (tests/test_gpu_codec_enc_ops.py, tests/test_gpu_whisper_ops.py): each formula below is the
# transformers / openai-whisper module the kernel cites, in plain torch at the dtype of its
# inputs, so one definition gives the fp64 reference and the fp32 evaluation that sets the bound.
FP32_FACTOR = 8   # a different summation order and the device expf / sinf / erff


def _cast(x, dt):
    return x.to(dt) if torch.is_tensor(x) and x.is_floating_point() else x


def fp64_and_fp32(formula, *args, **kw):
    """(the formula in fp64, max |the formula in fp32 on the CPU - that|), from the same fp32 inputs."""
    ref = formula(*[_cast(a, torch.float64) for a in args], **kw)
    lo = formula(*[_cast(a, torch.float32) for a in args], **kw)
    assert ref.dtype == torch.float64 and lo.dtype == torch.float32
    return ref, (lo.double() - ref).abs().max().item()


def fp32_op_error(tag, got, ref, err32):
    """The kernel's max error against fp64, printed beside the fp32 evaluation's own and the bound
    FP32_FACTOR x that one (which never looks at the kernel's output)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), tag
    err = (got - ref).abs().max().item()
    print(f"{tag}: kernel vs fp64 {err:.3e}, fp32 torch vs fp64 {err32:.3e}, bound {FP32_FACTOR * err32:.3e}")
    return err


def check_fp32_op(tag, got, ref, err32):
    """fp32_op_error, asserted: at most FP32_FACTOR x the fp32 evaluation's own error."""
    err = fp32_op_error(tag, got, ref, err32)
    assert err <= FP32_FACTOR * err32, (tag, err, err32)
    return err


def relkey_attention(qkv, qe, heads, L, R, shift=0):
    """[tf] Wav2Vec2BertSelfAttention.forward, position_embeddings_type "relative_key", from the
    projections: qkv [T][3 * 64 * heads] (q | k | v), qe [T][heads][L + R + 1] = q . distance
    embedding. shift: added to the distance index (a reference-only tooth: what a wrong index
    would compute)."""
    T, H = qkv.shape[0], 64 * heads
    q, k, v = (qkv[:, i * H:(i + 1) * H].reshape(T, heads, 64).transpose(0, 1) for i in range(3))
    scores = torch.matmul(q, k.transpose(-2, -1)) / 8.0
    distance = torch.arange(T).view(1, -1) - torch.arange(T).view(-1, 1)
    idx = (torch.clamp(distance, -L, R) + L + shift).clamp(0, L + R)
    rel = qe.transpose(0, 1).gather(2, idx[None].expand(heads, T, T))
    scores = scores + rel / 8.0
    out = torch.matmul(torch.softmax(scores, dim=-1), v)
    return out.transpose(0, 1).reshape(T, H)


def relkey_scores(qkv, qe, heads, L, R):
    """The fp64 scores [heads][T][T] of relkey_attention (for the marker margins)."""
    T, H = qkv.shape[0], 64 * heads
    q, k = (qkv[:, i * H:(i + 1) * H].double().reshape(T, heads, 64).transpose(0, 1) for i in range(2))
    distance = torch.arange(T).view(1, -1) - torch.arange(T).view(-1, 1)
    idx = torch.clamp(distance, -L, R) + L
    return (torch.matmul(q, k.transpose(-2, -1)) + qe.double().transpose(0, 1).gather(2, idx[None].expand(heads, T, T))) / 8.0


def aa_snake(x, alpha_log, beta_log, filt):
    """[tf] Xcodec2AntiAliasedActivation1d(Xcodec2SnakeBeta): UpSample1d(2, 12) -> SnakeBeta ->
    DownSample1d(2, 12), on x [T][C] time-major."""
    import torch.nn.functional as F
    h = x.t()[None]
    C = h.shape[1]
    f = filt.view(1, 1, 12).expand(C, -1, -1)
    h = F.pad(h, (5, 5), mode="replicate")
    h = 2 * F.conv_transpose1d(h, f, stride=2, groups=C)
    h = h[..., 15:-15]
    alpha = torch.exp(alpha_log)[None, :, None]
    beta = torch.exp(beta_log)[None, :, None]
    h = h + (1.0 / (beta + 0.000000001)) * torch.pow(torch.sin(h * alpha), 2)
    h = F.pad(h, (5, 6), mode="replicate")
    h = F.conv1d(h, f, stride=2, groups=C)
    return h[0].t().contiguous()


def conv_module_mid(p1, dw, ln_w, ln_b, eps):
    """[tf] Wav2Vec2BertConvolutionModule.forward between pointwise_conv1 and pointwise_conv2:
    GLU, left pad KW - 1, depthwise conv, LayerNorm, swish. p1 [T][2H], dw [H][KW] -> [T][H]."""
    import torch.nn.functional as F
    H, KW = dw.shape
    h = F.glu(p1.t()[None], dim=1)
    h = F.pad(h, (KW - 1, 0))
    h = F.conv1d(h, dw[:, None, :], groups=H)
    h = F.layer_norm(h.transpose(1, 2), (H,), ln_w, ln_b, eps)
    return F.silu(h)[0].contiguous()


def whisper_attention(Q, K, V, heads, causal, q_off, past=0):
    """whisper/model.py MultiHeadAttention.qkv_attention (head size 64: softmax(q k^T / 8) v);
    causal: query i sees keys [0, q_off + i + past] (past = 1: the reference-only tooth, a mask one
    key late). Q [Tq][64 * heads]; K, V [Tk][>= 64 * heads]."""
    Tq, Tk, H = Q.shape[0], K.shape[0], 64 * heads
    q = Q.reshape(Tq, heads, 64).transpose(0, 1)
    k = K[:, :H].reshape(Tk, heads, 64).transpose(0, 1)
    v = V[:, :H].reshape(Tk, heads, 64).transpose(0, 1)
    s = torch.matmul(q, k.transpose(-2, -1)) * 0.125
    if causal:
        hidden = torch.arange(Tk).view(1, -1) > torch.arange(Tq).view(-1, 1) + q_off + past
        s = s.masked_fill(hidden[None], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), v).transpose(0, 1).reshape(Tq, H)


def whisper_linear(X, W, bias, resid, gelu):
    """nn.Linear, then the exact (erf) nn.GELU of the MLP, then the block's residual add."""
    import torch.nn.functional as F
    y = F.linear(X, W, bias)
    if gelu:
        y = F.gelu(y)
    return y if resid is None else y + resid


def peaked_qkv(g, Tq, Tk, heads, marker, gain=9.0):
    """q [Tq][heads][64], k, v [Tk][heads][64]: every query is 20 u + noise for one unit direction
    u per head, so ordinary scores (q . k / 8) spread over about +-8 (sigma 2.7), and key
    `marker` is gain x u -- a score of gain / 8 x (20 +- 4) for every query, 8 or more above every
    other key's -- with V = +4: the running maximum moves when the marker's tile comes."""
    u = torch.randn(heads, 64, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    q = torch.randn(Tq, heads, 64, generator=g) + 20.0 * u
    k = torch.randn(Tk, heads, 64, generator=g)
    v = torch.randn(Tk, heads, 64, generator=g)
    k[marker] = gain * u
    v[marker] = 4.0
    return q.contiguous(), k.contiguous(), v.contiguous(), u

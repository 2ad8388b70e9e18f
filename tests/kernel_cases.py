"""Inputs, references and reference-only teeth shared by the kernel-level tests of the fast
path's encoder / prefill kernels: tests/test_gpu_attention_packed.py, test_gpu_rope_store.py
and test_gpu_norm_sources.py launch the kernels; tests/test_kernel_cases_cpu.py asserts, with
no GPU, what those tests rely on before they launch anything -- that a window one key longer or
shorter moves every marked query of the chosen seeds by ten times the bound, that a lost block
rescale moves the windowed block cases as far, that the slab values tell a slab order, and that
the share of RoPE pairs next to a bf16 tie is what the safe-set rule expects. Also the decode
attention call and its fp64 reference (tests/test_gpu_attention.py, test_gpu_attn_chunk_scores.py),
the eager (softcap) score of csrc/common.h fast_score restated in torch with the marked cases of
tests/test_gpu_attn_softcap.py (their teeth, too, asserted here from the references alone),
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
                          prepare=None, want_rc=0, softcap=0.0):
    """One t5g_attention_decode(_flash) call on random bf16 q / K / V (attn_inputs, one query
    per row); returns the output (fp64, [B][Hq][D]) and the host inputs. cap: cache slots per
    (row, kv head), default L; prepare(q, K, V) edits the inputs in place before the upload;
    want_rc != 0: the call must return that status and write nothing (returns None); softcap:
    None leaves the struct's field unset (the ctypes default), else it is passed through."""
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
    if softcap is not None:
        a.softcap = softcap
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


# ---------------------------------------------------------------------------
# decode attention with the eager score (softcap > 0): tests/test_gpu_attn_softcap.py
def _rbf(x):
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    return x.float().to(BF16).float()


def fast_score_ref(s_fp32, scale, softcap, drop=None):
    """csrc/common.h fast_score restated: from the fp32 dot product, x scale; or, softcap > 0,
    the five bf16 roundings of the eager score -- 0 bf16(q.k), 1 bf16(x scale), 2 bf16(/ softcap),
    3 bf16(tanh), 4 bf16(x softcap) -- every operation in fp32 (the tanh correctly rounded to
    fp32). drop: the rounding point left out (a reference-only tooth). Returns fp32."""
    s = s_fp32.float()
    sc = torch.tensor(scale, dtype=torch.float32)
    if not softcap > 0:
        return s * sc
    cap = torch.tensor(softcap, dtype=torch.float32)

    def r(i, x):
        return x if drop == i else _rbf(x)

    v = r(1, r(0, s) * sc)
    w = r(2, v / cap)
    return r(4, r(3, torch.tanh(w.double()).float()) * cap)


def bf16_tie_margin(v):
    """How far the fp64 values v lie from the nearest bf16 rounding tie, in bf16 steps (0 .. 0.5;
    0.5: on a bf16 value). As trig_safe measures it."""
    a = v.double().abs().clamp(min=2.0 ** -100)
    e = torch.floor(torch.log2(a))
    frac = torch.remainder(a / torch.exp2(e - 7), 1.0)
    return (frac - 0.5).abs()


def fast_score_margin(s_fp64, scale, softcap):
    """The smallest bf16_tie_margin over fast_score's five rounding points, each value computed
    in fp64 from the rounded value before it (the first from the fp64 dot product)."""
    sc = float(torch.tensor(scale, dtype=torch.float32))
    m = bf16_tie_margin(s_fp64)
    a = _rbf(s_fp64.double()).double() * sc
    m = torch.minimum(m, bf16_tie_margin(a))
    b = _rbf(a).double() / softcap
    m = torch.minimum(m, bf16_tie_margin(b))
    c = torch.tanh(_rbf(b).double())
    m = torch.minimum(m, bf16_tie_margin(c))
    d = _rbf(c).double() * softcap
    return torch.minimum(m, bf16_tie_margin(d))


SCORE_VARIANTS = ("restated", "exact", "nocap", "late_scale")


def decode_softcap_attention(q, K, V, lens, scale, softcap, window=0, variant="restated", drop=None):
    """fp64 softmax and P.V of each row's query over its keys [lo, lens[b]) (decode_exact_attention's
    range), on the scores of one variant of the softcap: "restated" the fp32 dot product through
    fast_score_ref (what the kernels are to compute), "exact" fp64 softcap * tanh(s * scale /
    softcap), and the two reference-only teeth "nocap" (s * scale: the softcap dropped) and
    "late_scale" (tanh(s / softcap) * softcap * scale: the softcap before the scale)."""
    assert variant in SCORE_VARIANTS and softcap > 0
    B, Hq, D = q.shape
    G = Hq // K.shape[1]
    out = torch.zeros(B, Hq, D, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        lo = max(0, L - window) if window > 0 else 0
        for h in range(Hq):
            s = K[b, h // G, lo:L].double() @ q[b, h].double()
            if variant == "restated":
                s = fast_score_ref(s.float(), scale, softcap, drop).double()   # drop: see fast_score_ref
            elif variant == "exact":
                s = softcap * torch.tanh(s * scale / softcap)
            elif variant == "nocap":
                s = s * scale
            else:
                s = torch.tanh(s / softcap) * softcap * scale
            out[b, h] = torch.softmax(s, 0) @ V[b, h // G, lo:L].double()
    return out


# The cases. Plain randn inputs give scores near +-1, where the softcap is almost the identity,
# so every row with two or more keys in range carries two markers per kv head h, along the
# query q^ of the group's first head (q head h * G): the first key in range is
# K = 50 q^ / (scale |q^|^2) with V = +4, the last K = 53 q^ / (scale |q^|^2) with V = -4 --
# scaled scores of 50 and 53, about 38.1 and 39.3 after the softcap, so the marked heads' outputs
# (about -2.2) hang on that gap. Every seed below has safe markers and teeth that hold
# (softcap_case asserts both; tests/test_kernel_cases_cpu.py runs it): should an edit here make
# one fail, another seed is the remedy, never a looser margin or bound.
SOFTCAP = 50.0
SOFTCAP_MARKS = (50.0, 53.0)
SOFTCAP_SAFE = 2.0 ** -10   # of a bf16 step, at every rounding point of a marker's score


def _sc(L, lens, seed, **kw):
    return dict(dict(L=L, lens=lens, seed=seed, window=0, causal=1, cap=L, Hq=8, Hkv=4, D=256, nan_past=False,
                     forms=(False, True), marks=None), **kw)


# The markers at 50 and 53 take one path through the five roundings (800 -> 50 -> 1 -> 0.7617 -> 38,
# 848 -> 53 -> 1.0625 -> 0.7852 -> 39.25), on which only a missing last rounding changes a
# bit: the spread cases give every (row, kv head) its own first marker score
# (marks[row * Hkv + head], the second 3 above it), chosen on the CPU so that the restated
# reference with any one rounding left out moves some marked head by ten times the bound.
# At head_dim 256 the scale is a power of two and roundings 0 and 1 are one rounding (leaving
# one of them out changes no bit); head_dim 128 tells them apart.
SPREAD_256 = (26.125, 27.125, 28.5, 30.125, 34.5, 38.0, 38.75, 39.5, 40.25, 41.25, 42.75, 43.5, 48.0, 49.5, 51.25, 53.25)
SPREAD_128 = (26.0, 27.125, 28.5, 30.125, 31.125, 32.5, 34.5, 38.0, 38.75, 39.5, 42.75, 43.5, 63.75, 65.0, 67.5, 36.0)
SPREAD_GAP = 1.5


SOFTCAP_CASES = {
    # chunk edges: rows of 2 and 64 keys (one chunk), 65 (a second chunk of one key) and L
    "edges65": _sc(65, [65, 65, 64, 2], 6500),
    "edges128": _sc(128, [128, 65, 64, 2], 12800),
    "edges191": _sc(191, [191, 65, 64, 2], 19100),
    # a 100-key window: chunks that start at key t - 99
    "window100": _sc(300, [300, 251, 101, 64], 30000, window=100),
    # the cross-attention shape: the per-op launch that stage A of the layer launch must equal
    "cross": _sc(64, [60, 64, 9, 2], 6000, causal=0),
    # NaN in K and V in every slot past each row's length, 70 slots past the longest row
    "nan_past": _sc(191, [191, 130, 65, 64], 700, cap=191 + 70, nan_past=True),
    # every instantiated (head_dim, group), 2 kv heads: both fast_score sites of attn.hip
    "geom64x2": _sc(70, [70, 64, 9, 1], 6420, Hq=4, Hkv=2, D=64),
    "geom128x2": _sc(70, [70, 64, 9, 1], 12820, Hq=4, Hkv=2, D=128),
    "geom256x1": _sc(70, [70, 64, 9, 1], 25610, Hq=2, Hkv=2, D=256),
    "geom256x2": _sc(70, [70, 64, 9, 1], 25620, Hq=4, Hkv=2, D=256),
    # 32 rows, flash form
    "rows32": _sc(130, [(130, 129, 65, 64, 2, 127, 70, 1)[i % 8] for i in range(32)], 3200, forms=(True,)),
    # a marker score of its own per (row, kv head): every rounding point of fast_score
    "spread256": _sc(150, [150, 65, 64, 2], 15000, marks=SPREAD_256),
    "spread128": _sc(150, [150, 65, 64, 2], 15001, D=128, marks=SPREAD_128),
}
SPREAD_DROPS = {"spread256": (2, 3), "spread128": (0, 1, 2, 3)}


def softcap_key_range(c, b):
    L = c["lens"][b]
    return (max(0, L - c["window"]) if c["window"] > 0 else 0), L


def softcap_marks(c, b, h):
    """The scaled scores planted on the first and the last key in range of (row b, kv head h)."""
    if c["marks"] is None:
        return SOFTCAP_MARKS
    base = c["marks"][b * c["Hkv"] + h]
    return base, base + SPREAD_GAP


def softcap_prepare(c):
    """prepare(q, K, V) of decode_attention_call for case c: the markers, then the NaN slots."""
    G = c["Hq"] // c["Hkv"]
    scale = float(torch.tensor(c["D"] ** -0.5, dtype=torch.float32))

    def prepare(q, K, V):
        for b in range(len(c["lens"])):
            lo, hi = softcap_key_range(c, b)
            if hi - lo >= 2:
                for h in range(c["Hkv"]):
                    qh = q[b, h * G].float()
                    s0, s1 = softcap_marks(c, b, h)
                    for key, score, v in ((lo, s0, 4.0), (hi - 1, s1, -4.0)):
                        K[b, h, key] = (score / scale * qh / qh.norm() ** 2).to(BF16)
                        V[b, h, key] = v
            if c["nan_past"]:
                K[b, :, hi:] = float("nan")
                V[b, :, hi:] = float("nan")
    return prepare


@functools.lru_cache(maxsize=None)
def softcap_case(name):
    """Inputs, the references of every score variant, the bound, and what the GPU test relies on,
    asserted here from the references alone: every marker's score is safe (more than
    SOFTCAP_SAFE of a bf16 step from a tie at each of fast_score's five rounding points, so the
    kernel's fp32 sum order cannot flip it), and "nocap" and "late_scale" each move every marked
    head of every marked row by at least ten times the (aten-order, the wider) bound; a rounding
    point left out moves them as the comment below says (50 / 53 cases: the last one; spread
    cases, which have no "nocap" / "late_scale" teeth: SPREAD_DROPS).
    Returns dict(c, q, K, V, ref: {variant: fp64 [B][Hq][D]}, bound: {flash: bound}, marked:
    [(row, q head)], move: {variant: smallest move over the marked heads; "drop<i>" of a spread
    case: marked heads moved by 4 bounds}, margin: smallest marker margin)."""
    c = SOFTCAP_CASES[name]
    B, G, D = len(c["lens"]), c["Hq"] // c["Hkv"], c["D"]
    scale = D ** -0.5
    q, K, V = attn_inputs(c["seed"], B, c["Hq"], c["Hkv"], D, B, c["cap"])
    softcap_prepare(c)(q, K, V)
    ref = {v: decode_softcap_attention(q, K, V, c["lens"], scale, SOFTCAP, c["window"], v) for v in SCORE_VARIANTS}
    assert bool(torch.isfinite(ref["restated"]).all()), name
    top = max(1.0, ref["restated"].abs().max().item())
    bound = {False: 2.0 ** -6 * top, True: 2.0 ** -7 * top}
    marked, margin = [], 0.5
    for b in range(B):
        lo, hi = softcap_key_range(c, b)
        if hi - lo < 2:
            continue
        for h in range(c["Hkv"]):
            marked.append((b, h * G))
            s = K[b, h, [lo, hi - 1]].double() @ q[b, h * G].double()
            margin = min(margin, fast_score_margin(s, scale, SOFTCAP).min().item())
            # the restated scores of the two markers: about 38 and 39.3 (spread cases: 22 to 46,
            # ordinary keys' e^-16 below), the last one the larger
            r = fast_score_ref(s.float(), scale, SOFTCAP)
            lim = (37.0, 40.0) if c["marks"] is None else (22.0, 46.0)
            assert lim[0] <= r[0].item() < r[1].item() <= lim[1], (name, b, h, r.tolist())
    assert len(marked) >= c["Hkv"] * (B - 1) // 2 and margin > SOFTCAP_SAFE, (name, c["seed"], margin)
    move = {}
    for v in ("nocap", "late_scale", "exact"):
        d = (ref[v] - ref["restated"]).abs().amax(-1)
        move[v] = min(d[b, h].item() for b, h in marked)
    for v in ("nocap", "late_scale"):
        # (a spread case's lower marker scores sit where the softcap is nearly linear: its teeth
        # are the rounding points, below)
        assert c["marks"] is not None or move[v] >= 10 * bound[False], (name, c["seed"], v, move[v], bound[False])
    # the restated reference with rounding point i left out. A kernel that left it out would sit
    # within its own error (at most the bound, were it otherwise right) of that reference, so a
    # move of 4 bounds leaves 3 to fail by. Spread cases: rounding i moves that far on at least
    # one marked head (a flipped marker moves its score by a whole bf16 step, 0.125 or 0.25).
    # The 50 / 53 cases: only the last rounding shows on their markers, as a part of a step
    # (38.086 -> 38, 39.258 -> 39.25): 0.108 on every marked head, 1.5 aten-order bounds or more.
    for i in SPREAD_DROPS.get(name, (4,)):
        d = (decode_softcap_attention(q, K, V, c["lens"], scale, SOFTCAP, c["window"], "restated", drop=i)
             - ref["restated"]).abs().amax(-1)
        if c["marks"] is None:
            move["drop%d" % i] = min(d[b, h].item() for b, h in marked)
            assert move["drop%d" % i] >= 1.5 * bound[False], (name, c["seed"], i, move["drop%d" % i], bound[False])
        else:
            move["drop%d" % i] = sum(d[b, h].item() >= 4 * bound[False] for b, h in marked)   # heads moved
            assert move["drop%d" % i] >= 1, (name, c["seed"], i)
    return dict(c=c, q=q, K=K, V=V, ref=ref, bound=bound, marked=marked, move=move, margin=margin)


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

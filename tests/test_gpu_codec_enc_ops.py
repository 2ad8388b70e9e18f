"""The codec encoder's row-wise kernels one at a time (xc2e_attention_relkey, xc2e_snake,
xc2e_conv_module_mid: the launch helpers xc2e_encode itself goes through, on caller buffers)
against the transformers module each restates, evaluated in fp64 from the same fp32 inputs
(tests/kernel_cases.py). The bound of every case is 8 x the error of the same formula evaluated
in fp32 by torch on the CPU -- taken from the two references, never from the kernel -- and both
errors are printed. Lengths run past the attention's 128-query block and 64-key tile, through
both clamps of the relative distance, either snake kernel form at every acoustic stage shape,
and the depthwise conv's causal edge and steady state."""
import pytest
import torch

from tests import kernel_cases as kc
from tests.engine_cases import need_gpu, ptr, stream

pytestmark = pytest.mark.gpu

HEADS = 2
REL = [(64, 8), (3, 2)]
ATTN_T = [1, 42, 64, 65, 128, 129, 200, 333]


def _fn(name):
    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.codec_enc import XC2E_SIGNATURES
    fn = getattr(_lib.lib(), name)
    fn.restype, fn.argtypes = XC2E_SIGNATURES[name]
    return fn


def _relkey_gpu(qkv, qe, L, R):
    """xc2e_attention_relkey on qkv [T][3 * 64 * HEADS]; three rows of NaN follow the T rows of
    qkv on the device (no key past T may count), and the rows after the output must stay NaN."""
    from t5gemma_tts_amd import _lib
    T, H = qkv.shape[0], 64 * HEADS
    qd = torch.cat([qkv, torch.full((3, 3 * H), float("nan"))]).cuda()
    ed = qe.contiguous().cuda()
    out = torch.full((T + 3, H), float("nan"), device="cuda")
    _lib.check(_fn("xc2e_attention_relkey")(ptr(qd), T, HEADS, ptr(ed), L, R, ptr(out), stream()), "attention_relkey")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[T:]).all())
    return out[:T]


def _relkey_inputs(seed, T, L, R, q_scale=1.0, qe_scale=4.0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3 * 64 * HEADS, generator=g)
    qkv[:, :64 * HEADS] *= q_scale
    qe = qe_scale * torch.randn(T, HEADS, L + R + 1, generator=g)
    return qkv.contiguous(), qe.contiguous()


@pytest.mark.parametrize("L,R", REL, ids=lambda v: str(v))
@pytest.mark.parametrize("T", ATTN_T)
def test_attention_relkey_vs_fp64(T, L, R):
    """Seeded random projections; (3, 2) clamps on both sides at every length above 4, (64, 8)
    on the left from T = 66 (three query blocks and six key tiles at T = 333).
    MI355X: kernel / fp32-torch error against fp64 at most 6.7e-7 / 6.7e-7 (T = 128), the worst
    ratio 1.8 (T = 42, (3, 2): 5.1e-7 / 2.9e-7); T = 1 is exact on both sides."""
    need_gpu()
    qkv, qe = _relkey_inputs(1000 + T, T, L, R)
    ref, err32 = kc.fp64_and_fp32(kc.relkey_attention, qkv, qe, HEADS, L, R)
    kc.check_fp32_op(f"attn_relkey T={T} L={L} R={R}", _relkey_gpu(qkv, qe, L, R), ref, err32)


def _tiles(T):
    """Marker keys of a T-frame utterance: in the first 64-key tile, the last full tile, and the
    ragged last tile -- those of them that exist and differ."""
    full, rag = T // 64, T % 64
    where = {"first": min(5, T - 1)}
    if full >= 2:
        where["last_full"] = 64 * (full - 1) + 37
    if rag and full >= 1:
        where["ragged"] = 64 * full + rag // 2
    return where


PEAKED = [(T, w) for T in (65, 129, 200, 333) for w in _tiles(T)]


@pytest.mark.parametrize("T,where", PEAKED, ids=lambda v: str(v))
def test_attention_relkey_peaked_marker(T, where):
    """Scores over about +-8 and one marker key whose score is 8 or more above every other key's
    for every query (asserted on the fp64 scores), V = +4, placed so that the running maximum
    rises in the first tile, the last full tile or the ragged last one: a lost or wrong
    exp(m_old - m_new) rescale leaves an output far from 4.
    MI355X: at most 3.6e-6 / 2.0e-6 (T = 333, first tile), the worst ratio 2.1 (T = 200, first
    tile: 2.9e-6 / 1.4e-6); margins 10.5 .. 12.6."""
    need_gpu()
    L, R = 64, 8
    key = _tiles(T)[where]
    g = torch.Generator().manual_seed(2000 + T)
    q, k, v, _ = kc.peaked_qkv(g, T, T, HEADS, key)
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).contiguous()
    qe = 4.0 * torch.randn(T, HEADS, L + R + 1, generator=g)
    s = kc.relkey_scores(qkv, qe, HEADS, L, R)
    others = s.clone()
    others[:, :, key] = float("-inf")
    margin = (s[:, :, key] - others.max(-1).values).min().item()
    spread = others[others > float("-inf")]
    print(f"T={T} marker key {key}: margin {margin:.2f}, other scores {spread.min().item():.1f} .. {spread.max().item():.1f}")
    assert margin >= 8.0, margin
    ref, err32 = kc.fp64_and_fp32(kc.relkey_attention, qkv, qe, HEADS, L, R)
    assert (ref - 4.0).abs().max().item() < 0.05      # the marker's V row, to e^-8
    kc.check_fp32_op(f"attn_relkey peaked T={T} {where}", _relkey_gpu(qkv, qe, L, R), ref, err32)


@pytest.mark.parametrize("L,R", REL, ids=lambda v: str(v))
def test_attention_relkey_distance_term_dominates(L, R):
    """q . k is scaled down to +-0.1 and q . E up to +-5, so the distance index decides the
    softmax: the reference with its index off by one (either way) moves by more than 1000 x the
    bound, asserted here on the references alone.
    MI355X: 3.0e-6 / 1.9e-6 at (64, 8), ratio 1.6."""
    need_gpu()
    T = 200
    qkv, qe = _relkey_inputs(3000 + L, T, L, R, q_scale=0.1, qe_scale=40.0)
    ref, err32 = kc.fp64_and_fp32(kc.relkey_attention, qkv, qe, HEADS, L, R)
    for shift in (-1, 1):
        moved = (kc.relkey_attention(qkv.double(), qe.double(), HEADS, L, R, shift=shift) - ref).abs().max().item()
        assert moved > 1000 * kc.FP32_FACTOR * err32, (shift, moved, err32)
    kc.check_fp32_op(f"attn_relkey qe-dominated L={L} R={R}", _relkey_gpu(qkv, qe, L, R), ref, err32)


# ----------------------------------------------------------------------------- snake
SNAKE_C = [1, 5, 48]
SNAKE_T = [1, 2, 5, 7, 8, 9, 12, 210, 1000]   # T = 1 is the shortest the reference's replicate pad takes


def _snake_inputs(C_, T, beta=None):
    from t5gemma_tts_amd.codec_enc import kaiser_sinc_filter
    g = torch.Generator().manual_seed(4000 + 13 * C_ + T)
    x = torch.randn(T, C_, generator=g)
    al = torch.rand(C_, generator=g) * 2 - 1
    bl = torch.rand(C_, generator=g) * 2 - 1 if beta is None else torch.full((C_,), float(beta))
    return x.contiguous(), al, bl, kaiser_sinc_filter().contiguous()


def _snake_gpu(x, al, bl, filt, form):
    from t5gemma_tts_amd import _lib
    T, C_ = x.shape
    xd, ad, bd, fd = x.cuda(), al.cuda(), bl.cuda(), filt.cuda()
    y = torch.full((T + 2, C_), float("nan"), device="cuda")
    _lib.check(_fn("xc2e_snake")(ptr(xd), T, C_, ptr(ad), ptr(bd), ptr(fd), ptr(fd), ptr(y), form, stream()), "snake")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[T:]).all())
    return y[:T]


@pytest.mark.parametrize("C_", SNAKE_C)
@pytest.mark.parametrize("T", SNAKE_T)
def test_snake_vs_fp64(T, C_):
    """The encoder's own dispatch (form 0: four outputs per thread at T = 8, 12, 1000, the
    per-output kernel elsewhere) and the per-output kernel at every T (form 1), each against fp64;
    where the dispatch takes the 4-wide kernel the two forms are bitwise equal, as
    aa_snake4_kernel's comment says.
    MI355X: at most 1.8e-6 / 1.3e-6 (T = 1000, C = 48), the worst ratio 2.5 (T = 9, C = 1:
    2.8e-7 / 1.1e-7); the two forms bitwise equal at T = 8, 12 and 1000 for every C."""
    need_gpu()
    x, al, bl, filt = _snake_inputs(C_, T)
    ref, err32 = kc.fp64_and_fp32(kc.aa_snake, x, al, bl, filt)
    y0 = _snake_gpu(x, al, bl, filt, 0)
    y1 = _snake_gpu(x, al, bl, filt, 1)
    kc.check_fp32_op(f"snake form 0 T={T} C={C_}", y0, ref, err32)
    kc.check_fp32_op(f"snake form 1 T={T} C={C_}", y1, ref, err32)
    if T % 4 == 0 and T >= 8:
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), (T, C_)


@pytest.mark.parametrize("T", [7, 12, 210, 1000])
def test_snake_tiny_beta_guard(T):
    """beta_log = -20: 1 / (e^-20 + 1e-9) = 3.3e8, the regime of the module's no_div_by_zero
    guard, where the fp32 sum e^-20 + 1e-9 and the sin^2 term's rounding carry the error; the
    bound scales with the fp32 reference's own error at that magnitude.
    MI355X: outputs of order 1e8; at most 1.22e+2 / 1.28e+2 (T = 1000), the worst ratio 1.5
    (T = 12: 64.6 / 42.0); the two forms bitwise equal at T = 12 and 1000."""
    need_gpu()
    x, al, bl, filt = _snake_inputs(5, T, beta=-20.0)
    ref, err32 = kc.fp64_and_fp32(kc.aa_snake, x, al, bl, filt)
    y0 = _snake_gpu(x, al, bl, filt, 0)
    y1 = _snake_gpu(x, al, bl, filt, 1)
    kc.check_fp32_op(f"snake beta -20 form 0 T={T}", y0, ref, err32)
    kc.check_fp32_op(f"snake beta -20 form 1 T={T}", y1, ref, err32)
    if T % 4 == 0 and T >= 8:
        assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)), T


# ----------------------------------------------------------------- conv module middle
@pytest.mark.parametrize("H", [128, 1024])
@pytest.mark.parametrize("T", [1, 30, 31, 32, 100])
def test_conv_module_mid_vs_fp64(T, H):
    """KW = 31: T = 1 .. 30 is all causal edge (t < KW - 1), 31 and 32 the first full windows,
    100 mostly steady state; H = 128 is half a block of threads, 1024 the real width.
    MI355X: at most 1.4e-6 / 1.6e-6 (T = 100, H = 1024), the worst ratio 1.5 (T = 1, H = 1024:
    1.1e-6 / 7.3e-7)."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    KW, eps = 31, 1e-5
    g = torch.Generator().manual_seed(5000 + T + H)
    p1 = torch.randn(T, 2 * H, generator=g).contiguous()
    dw = (torch.randn(H, KW, generator=g) / KW ** 0.5).contiguous()
    lw = 1.0 + 0.05 * torch.randn(H, generator=g)
    lb = 0.02 * torch.randn(H, generator=g)
    ref, err32 = kc.fp64_and_fp32(kc.conv_module_mid, p1, dw, lw, lb, eps)
    pd, dd, wd, bd = p1.cuda(), dw.cuda(), lw.cuda(), lb.cuda()
    out = torch.full((T + 2, H), float("nan"), device="cuda")
    _lib.check(_fn("xc2e_conv_module_mid")(ptr(pd), T, H, KW, ptr(dd), ptr(wd), ptr(bd), eps, ptr(out), stream()),
               "conv_module_mid")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[T:]).all())
    kc.check_fp32_op(f"conv_module_mid T={T} H={H}", out[:T], ref, err32)

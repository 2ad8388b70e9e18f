"""The Whisper text decoder's attention and linear dispatch one op at a time (whs_attention_op ->
dec_attention: the split + merge kernels for one query, the tiled kernel otherwise;
whs_linear_op -> dgemm: the GEMV for M <= 4, the tiled GEMM otherwise) against the openai-whisper
formulas in fp64 from the same fp32 inputs (tests/kernel_cases.py), at the lengths transcribe()
reaches: a self cache past 256 keys, causal query blocks at an offset, 1500 cross keys, K = 5120.
The bound of every case is 8 x the error of the same formula evaluated in fp32 by torch on the
CPU -- taken from the two references, never from the kernel -- and both errors are printed."""
import functools

import pytest
import torch

from tests import kernel_cases as kc
from tests.engine_cases import need_gpu, ptr, stream

pytestmark = pytest.mark.gpu

HEADS, H = 2, 128


@functools.lru_cache(maxsize=None)
def _model():
    """A recognizer at the tiny test dims (two text heads); the ops use its head count and its
    split workspace, none of its weights."""
    from t5gemma_tts_amd import whisper_asr as w
    d = w.dims_tiny()
    assert d.n_text_head == HEADS and d.n_text_ctx == 448 and d.n_audio_ctx == 1500
    return w.WhisperModel(d, w.synthetic_weights(d, 41), device="cuda:0", max_seconds=1.0)


def _attn_gpu(Q, K, V, Tk, causal, q_off, ldkv=H):
    """whs_attention_op on Q [Tq][H] and the first Tk rows of K / V, stored with row stride ldkv;
    the rows after Tk hold a key that would win every softmax and NaN values (they must not be
    read into the result), and the rows after the output must stay NaN."""
    from t5gemma_tts_amd import _lib
    m = _model()
    Tq = Q.shape[0]
    Kd = torch.full((Tk + 3, ldkv), 1e3)
    Vd = torch.full((Tk + 3, ldkv), float("nan"))
    Kd[:Tk, :H], Vd[:Tk, :H] = K[:Tk], V[:Tk]
    Vd[:Tk, H:] = 0.0
    Qd, Kd, Vd = Q.contiguous().cuda(), Kd.cuda(), Vd.cuda()
    out = torch.full((Tq + 2, H), float("nan"), device="cuda")
    rc = m.L.whs_attention_op(m.h, ptr(Qd), ptr(Kd), ptr(Vd), ldkv, Tq, Tk, causal, q_off, ptr(out), stream())
    _lib.check(rc, "whs_attention_op")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[Tq:]).all())
    return out[:Tq]


def _rand_qkv(seed, Tq, Tk):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(Tq, H, generator=g), torch.randn(Tk, H, generator=g), torch.randn(Tk, H, generator=g))


DEC_TK = [1, 63, 255, 256, 257, 448, 1500]


@pytest.mark.parametrize("Tk", DEC_TK)
def test_attention_one_query_vs_fp64(Tk):
    """Tq = 1, the split + merge kernels: one split to 256 keys, a second of a single key at 257,
    a ragged second at 448 (the last cache row), six at the 1500 cross keys. The self-cache
    lengths run as the decoder calls them (causal, q_off = Tk - 1), 1500 as cross attention.
    MI355X: kernel / fp32-torch error against fp64 at most 9.7e-8 / 1.5e-7 (Tk = 448), every
    ratio below 1; Tk = 1 is exact on both sides."""
    need_gpu()
    Q, K, V = _rand_qkv(6000 + Tk, 1, Tk)
    causal = int(Tk <= 448)
    ref, err32 = kc.fp64_and_fp32(kc.whisper_attention, Q, K, V, HEADS, causal, Tk - 1)
    kc.check_fp32_op(f"whs attention Tq=1 Tk={Tk}", _attn_gpu(Q, K, V, Tk, causal, Tk - 1 if causal else 0), ref, err32)


TILED = [(3, 3, 1, 0), (4, 10, 1, 6), (5, 70, 1, 65), (130, 130, 1, 0), (129, 333, 1, 204), (7, 1500, 0, 0)]


@pytest.mark.parametrize("Tq,Tk,causal,q_off", TILED, ids=lambda v: str(v))
def test_attention_query_block_vs_fp64(Tq, Tk, causal, q_off):
    """Tq > 1, the tiled kernel: prefill (q_off = 0) past one query block and one key tile, chunks
    at an offset, and seven queries over 1500 keys at the encoder's row stride (3 x 128). In the
    causal cases the key just after the middle query's range, q_off + i + 1, is aimed at that
    query (a score of about 8) with V = +4: it must not count -- the reference with its mask one
    key late moves by more than 1000 x the bound, asserted on the references alone.
    MI355X: at most 5.2e-7 / 4.3e-7 ((130, 130, 1, 0)), the worst ratio 2.5 ((7, 1500, 0, 0):
    1.5e-7 / 6.2e-8)."""
    need_gpu()
    Q, K, V = _rand_qkv(7000 + Tq + Tk, Tq, Tk)
    i0 = Tq // 2
    if causal:
        key = q_off + i0 + 1
        assert key < Tk
        qh = Q[i0].view(HEADS, 64)
        K[key] = (8.0 * qh / qh.norm(dim=-1, keepdim=True)).reshape(H)
        V[key] = 4.0
    ref, err32 = kc.fp64_and_fp32(kc.whisper_attention, Q, K, V, HEADS, causal, q_off)
    if causal:
        late = kc.whisper_attention(Q.double(), K.double(), V.double(), HEADS, causal, q_off, past=1)
        moved = (late[i0] - ref[i0]).abs().max().item()
        assert moved > 1000 * kc.FP32_FACTOR * err32, (moved, err32)
    got = _attn_gpu(Q, K, V, Tk, causal, q_off, ldkv=H if causal else 3 * H)
    kc.check_fp32_op(f"whs attention Tq={Tq} Tk={Tk} causal={causal} q_off={q_off}", got, ref, err32)


def _marker_keys(Tk, tile):
    """Marker keys among Tk keys in tiles (or splits) of `tile`: first, last full, ragged last."""
    full, rag = Tk // tile, Tk % tile
    where = {"first": min(5, Tk - 1)}
    if full >= 2:
        where["last_full"] = tile * (full - 1) + tile // 2 + 5
    if rag and full >= 1:
        where["ragged"] = tile * full + rag // 2
    return where


PEAKED = [(1, Tk, 1, Tk - 1, "ragged") for Tk in (257, 448)] + [(1, 1500, 0, 0, "ragged"), (1, 1500, 0, 0, "last_full")] + \
    [(Tq, Tk, c, o, w) for Tq, Tk, c, o in TILED[3:] for w in ("first", "last_full", "ragged")]


@pytest.mark.parametrize("Tq,Tk,causal,q_off,where", PEAKED, ids=lambda v: str(v))
def test_attention_peaked_marker(Tq, Tk, causal, q_off, where):
    """Scores over about +-8 and one marker key whose score is 8 or more above every other key's
    for every query that sees it (asserted on the fp64 scores), V = +4, placed in the first tile,
    the last full tile or the ragged last one (Tq = 1: in the last 256-key split, one key long at
    257), so the running maximum -- the merge's maximum -- moves late.
    MI355X: at most 3.3e-6 / 2.7e-6 ((129, 333), ragged tile), the worst ratio 1.6 ((130, 130),
    first tile: 2.0e-6 / 1.2e-6); margins 11.6 .. 16.3."""
    need_gpu()
    key = _marker_keys(Tk, 256 if Tq == 1 else 64)[where]
    g = torch.Generator().manual_seed(8000 + Tq + Tk)
    q, k, v, _ = kc.peaked_qkv(g, Tq, Tk, HEADS, key)
    Q, K, V = q.reshape(Tq, H), k.reshape(Tk, H), v.reshape(Tk, H)
    s = torch.matmul(q.double().transpose(0, 1), k.double().transpose(0, 1).transpose(-2, -1)) * 0.125   # [h][Tq][Tk]
    last = torch.arange(Tq).view(-1, 1) + q_off if causal else torch.full((Tq, 1), Tk - 1)
    seen = torch.arange(Tk).view(1, -1) <= last   # [Tq][Tk]
    s = s.masked_fill(~seen[None], float("-inf"))
    sees = seen[:, key]
    assert bool(sees.any())
    others = s.clone()
    others[:, :, key] = float("-inf")
    margin = (s[:, sees, key] - others[:, sees].max(-1).values).min().item()
    print(f"Tq={Tq} Tk={Tk} marker key {key}: {int(sees.sum())} queries see it, margin {margin:.2f}")
    assert margin >= 8.0, margin
    ref, err32 = kc.fp64_and_fp32(kc.whisper_attention, Q, K, V, HEADS, causal, q_off)
    assert (ref[sees] - 4.0).abs().max().item() < 0.05
    got = _attn_gpu(Q, K, V, Tk, causal, q_off)
    kc.check_fp32_op(f"whs attention peaked Tq={Tq} Tk={Tk} {where}", got, ref, err32)


# ------------------------------------------------------------------------------ linear
SHAPES = [(128, 128), (1001, 512), (130, 2052), (64, 5120), (37, 130)]
GUARD = 64


def linear_supported(M, K):
    """dgemm's two paths: the GEMV takes M <= 4 rows at K % 4 == 0 (any number of 2048-wide
    passes, a ragged last one included); everything else goes to the tiled GEMM, which is built
    for K % 32 == 0 and refuses other K before it launches (include/whisper.h)."""
    return (M <= 4 and K % 4 == 0) or K % 32 == 0


@pytest.mark.parametrize("N,K", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("M", [1, 2, 3, 4, 5])
def test_linear_vs_fp64(M, N, K):
    """Every (bias, resid, epi) combination per shape: ragged N (1001, 130, 37 against 16 outputs
    per block), one GEMV pass (K <= 512), two with a one-float4 remainder (2052), three (5120,
    the real fc2), and M = 5 on the tiled GEMM. Y sits between NaN guards that must stay NaN.
    K = 2052 at M = 5 and K = 130 at every M fall to the tiled GEMM, which refuses K % 32 != 0
    with -1: there the call must return -1 and write nothing.
    MI355X: the GEMV (M <= 4) at most 6.6e-7 / 1.4e-6 (M = 4, (130, 2052)), the worst ratio 1.6.
    The tiled GEMM (M = 5) 1.1e-6 / 9.1e-7 at K = 128, 1.8e-6 / 1.2e-6 at K = 512 and 1.0e-6 / 1.1e-6
    at K = 5120, every ratio at most 1.5. With one fp32 accumulator per output over all of K
    the K = 5120 case stood at 6.4e-6 .. 6.7e-6 and missed the bound in two combinations (8.4 x the
    fp32 evaluation's 7.96e-7); gemm_f32_kernel now adds 256-wide partial sums."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    m = _model()
    g = torch.Generator().manual_seed(9000 + 7 * M + N + K)
    X = torch.randn(M, K, generator=g)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).contiguous()
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    Xd, Wd, bd, rd = X.cuda(), W.cuda(), b.cuda(), r.cuda()
    worst, missed = (0.0, 0.0), []
    for bias in (None, b):
        for resid in (None, r):
            for epi in (0, 4):
                buf = torch.full((GUARD + M * N + GUARD,), float("nan"), device="cuda")
                Y = buf[GUARD:GUARD + M * N]
                rc = m.L.whs_linear_op(ptr(Xd), M, ptr(Wd), N, K, ptr(bd) if bias is not None else None,
                                       ptr(rd) if resid is not None else None, epi, ptr(Y), stream())
                torch.cuda.synchronize()
                tag = f"whs linear M={M} N={N} K={K} bias={bias is not None} resid={resid is not None} epi={epi}"
                if not linear_supported(M, K):
                    assert rc == -1, (tag, rc)
                    assert bool(torch.isnan(buf).all()), tag
                    continue
                _lib.check(rc, "whs_linear_op")
                assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + M * N:]).all()), tag
                ref, err32 = kc.fp64_and_fp32(kc.whisper_linear, X, W, bias, resid, epi == 4)
                err = kc.fp32_op_error(tag, Y.view(M, N), ref, err32)
                worst = max(worst, (err, err32))
                if err > kc.FP32_FACTOR * err32:      # every combination is measured before the assert
                    missed.append((tag, err, err32))
    print(f"whs linear M={M} N={N} K={K}: worst kernel error {worst[0]:.3e} (fp32 torch {worst[1]:.3e})")
    assert not missed, missed

"""FP8 e4m3 decode weights on the GPU, kernel level (csrc/fp8.hip, csrc/gemv.hip): the
quantiser against its torch restatement, the kernels' convert on every code, and the P8
register-X GEMV against the bf16 GEMV on the P16 image of W_q -- all bit for bit (power-of-two
row scales make 2^e * code exactly bf16, so no tolerance is needed or used)."""
import ctypes as C

import pytest
import torch

from tests.engine_cases import need_gpu, ptr, stream
from tests.fixture_cases import planted_matrix

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
DEV = "cuda:0"


def _quantize(W, want_wq=True):
    """(rc, p8, scale, wq) of t5g_quantize_weight_fp8 on a device copy of W."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    N, K = W.shape
    Wd = W.to(DEV, BF16).contiguous()
    p8 = torch.full((L.t5g_fp8_packed_bytes(N, K),), 0x55, dtype=torch.uint8, device=DEV)
    scale = torch.full((-(-N // 16) * 16,), -7.0, dtype=torch.float32, device=DEV)
    wq = torch.full((N, K), 9.0, dtype=BF16, device=DEV) if want_wq else None
    rc = L.t5g_quantize_weight_fp8(ptr(Wd), N, K, K, ptr(p8), ptr(scale), ptr(wq), stream(DEV))
    return rc, p8, scale, wq


def _unpack(p8, scale, N, K):
    from t5gemma_tts_amd import _lib
    out = torch.full((N, K), 9.0, dtype=BF16, device=DEV)
    _lib.check(_lib.lib().t5g_fp8_unpack(ptr(p8), ptr(scale), N, K, ptr(out), stream(DEV)), "fp8_unpack")
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def test_all_codes_round_trip_through_the_kernels_convert():
    """16 rows x 256: row r holds every finite e4m3 value (the two NaN slots 0) times 2^e_r.
    Quantise, then unpack through the kernels' own convert: the input, bit for bit -- every
    code, subnormals included, and each row scale as the convert's scale operand."""
    need_gpu()
    vals = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    vals[0x7F] = 0.0
    vals[0xFF] = 0.0
    es = [(-20, -7, 0, 3)[r % 4] for r in range(16)]
    W = torch.stack([vals * 2.0 ** e for e in es]).to(BF16)
    assert torch.equal(W.float(), torch.stack([vals * 2.0 ** e for e in es]))   # exactly bf16
    rc, p8, scale, wq = _quantize(W)
    assert rc == 0
    assert scale.cpu().tolist() == [2.0 ** e for e in es]
    assert torch.equal(_bits(_unpack(p8, scale, 16, 256)), _bits(W))
    assert torch.equal(_bits(wq), _bits(W))


@pytest.mark.parametrize("N,K", [(40, 96), (208, 2304)])
def test_device_quantiser_equals_the_restatement(N, K):
    need_gpu()
    from t5gemma_tts_amd.weights import quantize_fp8_rows
    W = planted_matrix(N, K, 11 + N)
    codes, scale_ref, wq_ref = quantize_fp8_rows(W)
    rc, p8, scale, wq = _quantize(W)
    assert rc == 0
    NP = -(-N // 16) * 16
    s = scale.cpu()
    assert torch.equal(s[:N].view(torch.int32), scale_ref.view(torch.int32))
    assert bool((s[N:] == 1.0).all()) and s.numel() == NP            # padded rows: scale 1 ...
    assert torch.equal(_bits(wq), _bits(wq_ref))
    assert torch.equal(_bits(_unpack(p8, scale, N, K)), _bits(wq_ref))
    # the P8 image itself: fragment (g, kb), lane l = row l % 16, k 8 (l / 16) .. + 7
    img = p8.cpu().view(NP // 16, K // 32, 4, 16, 8)                 # [g][kb][l / 16][l % 16][8]
    rows = img.permute(0, 3, 1, 2, 4).reshape(NP, K)
    assert torch.equal(rows[:N], codes)
    assert not bool(rows[N:].any())                                  # ... and codes 0
    # without the W_q image
    rc2, p8b, scale_b, _ = _quantize(W, want_wq=False)
    assert rc2 == 0 and torch.equal(p8b.cpu(), p8.cpu()) and torch.equal(scale_b.cpu(), s)


def test_device_quantiser_refuses_a_non_finite_weight():
    need_gpu()
    from t5gemma_tts_amd import _lib
    W = planted_matrix(40, 96, 5)
    W[17, 40] = float("inf")
    rc, *_ = _quantize(W)
    assert rc == -1
    with pytest.raises(ValueError):
        _lib.check(rc, "quantize_weight_fp8")


# (epi, K, N, splits, nw, un, Ms): the decode step's register-X launches at a handful of groups
GEMV_CASES = [
    (4, 2304, 208, 2, 12, 0, (1, 8, 16, 17, 32)),   # q|k|v / cross-q: 2 slices of 36 k-steps
    (4, 2048, 208, 4, 8, 0, (8, 32)),               # o-projection: 4 slices of 16
    (4, 9216, 208, 8, 12, 0, (8, 19)),              # down: 8 slices of 36
    (3, 2304, 416, 1, 12, -1, (1, 8, 32)),          # gate/up GeGLU, every unit's weights up front
    (1, 2304, 200, 1, 4, 8, (8, 32)),               # the head: bias, a ragged last group
]
_W = {}


def _weights(N, K):
    """(P8, scale, P16 of W_q) of a seeded [N][K] matrix, made once per shape."""
    from t5gemma_tts_amd import _lib
    if (N, K) not in _W:
        L = _lib.lib()
        g = torch.Generator().manual_seed(N * 7 + K)
        W = (torch.randn(N, K, generator=g) * 0.02).to(BF16)
        rc, p8, scale, wq = _quantize(W)
        assert rc == 0
        p16 = torch.zeros(L.t5g_packed_bytes(N, K) // 2, dtype=BF16, device=DEV)
        _lib.check(L.t5g_pack_weight(ptr(wq), N, K, K, ptr(p16), stream(DEV)), "pack")
        _W[(N, K)] = (p8, scale, p16)
    return _W[(N, K)]


def _run(fp8, epi, M, N, K, splits, nw, un, X, bias, max_grid=0):
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    p8, scale, p16 = _weights(N, K)
    n_out = N // 2 if epi == 3 else N
    Y = torch.full((splits, M, n_out), 7.0, dtype=torch.float32 if epi == 4 else BF16, device=DEV)
    a = _lib.GemvArgs()
    a.M, a.K, a.N, a.epi, a.pro, a.nw, a.un = M, K, N, epi, 0, nw, un
    a.X, a.ldx, a.Y, a.ldy, a.splits, a.layout, a.max_grid = X.data_ptr(), K, Y.data_ptr(), n_out, splits, 1, max_grid
    a.bias = bias.data_ptr() if bias is not None else None
    if fp8:
        a.W = p8.data_ptr()
        _lib.check(L.t5g_gemv_fp8(C.byref(a), ptr(scale), stream(DEV)), "gemv_fp8")
    else:
        a.W = p16.data_ptr()
        _lib.check(L.t5g_gemv(C.byref(a), stream(DEV)), "gemv")
    torch.cuda.synchronize()
    return Y.cpu()


@pytest.mark.parametrize("epi,K,N,splits,nw,un,M", [c[:6] + (m,) for c in GEMV_CASES for m in c[6]])
def test_gemv_fp8_bitwise_equals_bf16_gemv_on_wq(epi, K, N, splits, nw, un, M):
    need_gpu()
    g = torch.Generator().manual_seed(1000 + M + K)
    X = torch.randn(M, K, generator=g).to(BF16).to(DEV)
    bias = (torch.randn(N, generator=g) * 0.1).to(BF16).to(DEV) if epi == 1 else None
    got = _run(True, epi, M, N, K, splits, nw, un, X, bias)
    ref = _run(False, epi, M, N, K, splits, nw, un, X, bias)
    assert bool(torch.isfinite(ref.float()).all()) and float(ref.float().abs().max()) > 0
    view = torch.int32 if epi == 4 else torch.int16
    assert torch.equal(got.view(view), ref.view(view))
    if M == 8 and K == 2304:
        # grid invariance: 100 blocks per launch instead of one per CU, and few enough blocks
        # that each streams several units (the double-buffered unit loop, 5 to 10 units a block)
        for cap in (100, 2 * splits if epi != 3 else 3):
            capped = _run(True, epi, M, N, K, splits, nw, un, X, bias, max_grid=cap)
            assert torch.equal(capped.view(view), got.view(view)), cap

"""FP8 e4m3 decode weights, the parts that need no GPU: the quantiser rule restated in torch
(weights.quantize_fp8_rows; the device kernel is compared with it bit for bit in
tests/test_gpu_fp8_gemv.py), the P8 size, the host-side shape checks of t5g_gemv_fp8 and the
CLI's flag validation."""
import ctypes as C

import pytest
import torch

from tests.fixture_cases import planted_matrix

BF16 = torch.bfloat16


@pytest.mark.parametrize("N,K", [(40, 96), (208, 2304)])
def test_quantize_fp8_rows_properties(N, K):
    from t5gemma_tts_amd.weights import quantize_fp8_rows
    W = planted_matrix(N, K, 11 + N)
    codes, scale, wq = quantize_fp8_rows(W)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K)
    assert scale.dtype == torch.float32 and scale.shape == (N,) and wq.dtype == BF16
    assert not bool(((codes & 0x7F) == 0x7F).any())          # never the NaN codes 0x7F / 0xFF
    q = codes.view(torch.float8_e4m3fn).float()
    assert bool(torch.isfinite(q).all()) and float(q.abs().max()) <= 448.0
    m, _ = torch.frexp(scale)
    assert bool((m == 0.5).all())                              # exact powers of two
    assert torch.equal(wq.float(), q * scale[:, None])         # W_q = 2^e q ...
    assert torch.equal(wq.float().to(BF16).float(), wq.float())   # ... and exactly bf16
    # the rule: the smallest e >= -100 with amax 2^-e <= 448 (e = 0 for the zero row)
    amax = W.float().abs().amax(1)
    nz = amax > 0
    assert bool((amax[nz] / scale[nz] <= 448.0).all())
    assert bool(((amax[nz] / (scale[nz] / 2) > 448.0) | (scale[nz] == 2.0 ** -100)).all())
    assert float(scale[3]) == 1.0 and not bool(codes[3].any())
    assert float(scale[5]) == 2.0 ** -3 and float(scale[6]) == 2.0 ** -2
    assert float(wq[9, 0]) == 3.0
    # every element is within half an e4m3 step of its row's scaled value (RNE): step 2^-9 in the
    # subnormals, 2^(floor(log2 |v|) - 3) above
    v = W.float() / scale[:, None]
    step = torch.where(v.abs() < 2.0 ** -6, torch.tensor(2.0 ** -9),
                       2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -6))) - 3))
    assert bool(((q - v).abs() <= step / 2).all())
    # quantising W_q again is a fixed point: the same W_q bit for bit. Codes and scales repeat
    # too wherever the row's largest value did not round DOWN onto 448 (= 1.75 * 2^8), where
    # the rule's own e for W_q is one smaller: then scale halves and the codes name the same
    # values one binade up. The planted 464 row is such a row (232 is the tie 224 | 240 -> 224).
    c2, s2, wq2 = quantize_fp8_rows(wq)
    assert torch.equal(wq2.view(torch.int16), wq.view(torch.int16))
    q2 = c2.view(torch.float8_e4m3fn).float()
    assert torch.equal(q2 * s2[:, None], q * scale[:, None])
    same = s2 == scale
    halved = (s2 == scale / 2) & (q.abs().amax(1) == 224.0)
    assert bool((same | halved).all())
    assert torch.equal(c2[same], codes[same])
    assert bool(halved[6]) and int(halved.sum()) < N // 4


def test_quantize_fp8_rows_boundaries_and_errors():
    from t5gemma_tts_amd.weights import quantize_fp8_rows
    for amax, e in ((448.0, 0), (449.0, 0), (464.0, 1), (896.0, 1)):   # bf16(449) = 448
        W = torch.full((1, 32), 0.5, dtype=BF16)
        W[0, 3] = amax
        assert float(quantize_fp8_rows(W)[1][0]) == 2.0 ** e, amax
    tiny = torch.full((1, 32), 2.0 ** -120, dtype=BF16)
    assert float(quantize_fp8_rows(tiny)[1][0]) == 2.0 ** -100    # the exponent floor
    bad = torch.zeros(2, 32, dtype=BF16)
    bad[1, 4] = float("inf")
    with pytest.raises(ValueError):
        quantize_fp8_rows(bad)


def test_fp8_rounded_state_dict_replaces_exactly_the_quantised_set():
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.weights import (fp8_quantized_names, fp8_rounded_state_dict, quantize_fp8_rows,
                                         synthetic_weights)
    cfg = named_config("tiny")
    sd = synthetic_weights(cfg, 3)
    out = fp8_rounded_state_dict(cfg, sd)
    names = set(fp8_quantized_names(cfg))
    assert set(out) == set(sd) and names <= set(sd)
    assert "predict_layer.0.2.weight" in names and "predict_layer.0.0.weight" not in names
    assert not any("encoder" in n or "cross_attn.k_proj" in n or "cross_attn.v_proj" in n for n in names)
    changed = 0
    for k in sd:
        if k in names:
            assert torch.equal(out[k], quantize_fp8_rows(sd[k])[2]), k
            changed += int(not torch.equal(out[k], sd[k]))
        else:
            assert out[k] is sd[k], k
    assert changed == len(names)


@pytest.mark.parametrize("N,K", [(16, 32), (200, 2304), (65541, 2304)])
def test_fp8_packed_bytes(N, K):
    from t5gemma_tts_amd import _lib
    assert _lib.lib().t5g_fp8_packed_bytes(N, K) == 16 * -(-N // 16) * K
    assert _lib.lib().t5g_fp8_packed_bytes(N, K + 1) < 0


@pytest.mark.parametrize("layout,M,K,splits,epi,nw", [
    (0, 8, 2304, 1, 0, 8),     # layout 0 (the LDS-staged GEMV) has no P8 form
    (1, 8, 96, 1, 0, 4),       # K = 96: not a k-step count the register-X kernel is built for
    (1, 33, 2304, 1, 0, 12),   # M = 33: past two 16-row tiles
])
def test_gemv_fp8_rejects_unsupported_shapes(layout, M, K, splits, epi, nw):
    """t5g_gemv_fp8 decides on the host, before any launch, like t5g_gemv -- and with the same
    code t5g_gemv gives an unbuilt layout-1 shape."""
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    a = _lib.GemvArgs()
    a.M, a.K, a.N, a.epi, a.pro, a.nw, a.un = M, K, 2304, epi, 0, nw, 8
    a.X, a.ldx, a.Y, a.ldy, a.splits, a.layout, a.max_grid = 16, K, 16, 2304, splits, layout, 0
    a.W = 16   # never dereferenced: every case is rejected before a launch
    rc = L.t5g_gemv_fp8(C.byref(a), C.c_void_p(16), None)
    assert rc < 0
    b = _lib.GemvArgs.from_buffer_copy(a)
    b.layout = 1
    if layout == 1:
        assert rc == L.t5g_gemv(C.byref(b), None)


def test_run_inference_rejects_unknown_weight_format(monkeypatch):
    from t5gemma_tts_amd import cli

    def no_load(*a, **k):
        raise AssertionError("nothing may be loaded for an unknown weight_format")
    monkeypatch.setattr(cli, "load_model", no_load)
    monkeypatch.setattr(cli, "load_codec", no_load)
    with pytest.raises(ValueError, match="weight_format"):
        cli.run_inference(target_text="hi", synthetic="tiny", weight_format="fp4")


def test_engine_refuses_unknown_format_and_unsupported_widths():
    """Checked before the GPU is touched: an unknown format, and FP8 on a config whose widths
    the decode GEMV sites are not built for."""
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import fp8_supported
    cfg = named_config("tiny")
    assert not fp8_supported(cfg)
    with pytest.raises(ValueError, match="weight_format"):
        T5GemmaTTSEngine(cfg, {}, weight_format="fp4")
    with pytest.raises(ValueError, match="fp8"):
        T5GemmaTTSEngine(cfg, {}, weight_format="fp8")

"""The hipEvent timing hooks (csrc/engine_hooks.hip; bench.py --full prices its rooflines with
them) on engine_cases.mid_engine(32), as in test_gpu_fused.py (true 2b-2b widths, 2 + 2 layers, max_text
64, max_audio 128): after a short generate() the three decode hooks return OK with a finite
positive time at 3 and at 16 rows, t5g_time_decode_layer refuses 17 rows, a hook leaves the
decode state marked invalid (t5g_decode then returns T5G_EINVAL), and a fresh generate() with the
same seeds still gives the tokens it gave before the hooks ran. t5g_time_gemm / t5g_time_gemv
once each at the smallest shape of test_gpu_gemv.py."""
import ctypes as C
import math

import pytest
import torch

from tests.engine_cases import default_params, mid_engine, need_gpu, stream, utterances

pytestmark = pytest.mark.gpu

ITERS = 4   # the decode hooks round it up to whole rotations over the layers
T5G_EINVAL, T5G_EUNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def mid():
    need_gpu()
    return mid_engine(32)


@pytest.mark.parametrize("B", [3, 16])
def test_decode_hooks_time_and_leave_generate_unchanged(mid, B):
    from t5gemma_tts_amd import _lib
    cfg, eng = mid
    L = _lib.lib()
    utts = utterances(cfg, B, 60 + B)
    p = default_params()
    seeds = list(range(700, 700 + B))
    before = eng.generate(utts, p, seeds=seeds)
    assert sum(len(g) for g in before["gen"]) > B
    st = stream()
    us, keys = C.c_float(0.0), C.c_float(0.0)
    assert L.t5g_time_decode_step(eng.h, ITERS, st, C.byref(us)) == 0
    assert math.isfinite(us.value) and us.value > 0, us.value
    us.value = 0.0
    assert L.t5g_time_decode_mlp(eng.h, B, ITERS, st, C.byref(us)) == 0
    assert math.isfinite(us.value) and us.value > 0, us.value
    us.value = 0.0
    assert L.t5g_time_decode_layer(eng.h, B, ITERS, st, C.byref(us), C.byref(keys)) == 0
    assert math.isfinite(us.value) and us.value > 0, us.value
    assert math.isfinite(keys.value) and keys.value > 0, keys.value
    # the hooks re-ran launches on the live decode state: the call cannot be continued
    assert L.t5g_decode(eng.h, 1, 0, st) == T5G_EINVAL
    after = eng.generate(utts, p, seeds=seeds)
    for b in range(B):
        assert after["gen"][b].tolist() == before["gen"][b].tolist(), b


def test_decode_layer_hook_refuses_17_rows(mid):
    from t5gemma_tts_amd import _lib
    _, eng = mid
    us, keys = C.c_float(0.0), C.c_float(0.0)
    rc = _lib.lib().t5g_time_decode_layer(eng.h, 17, ITERS, stream(), C.byref(us), C.byref(keys))
    assert rc == T5G_EUNSUPPORTED


def test_time_gemm_and_gemv_smallest_shape():
    need_gpu()
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    M, N, K = 3, 192, 64   # test_gpu_gemv.py CASES: tiny widths, most lanes idle
    g = torch.Generator(device="cpu").manual_seed(9)
    W = (torch.randn(N, K, generator=g) * 0.02).to(torch.bfloat16).cuda()
    X = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()
    st = stream()
    Wp = torch.empty(L.t5g_packed_bytes(N, K) // 2, dtype=torch.bfloat16, device="cuda")
    assert L.t5g_pack_weight(C.c_void_p(W.data_ptr()), N, K, K, C.c_void_p(Wp.data_ptr()), st) == 0
    arr = (C.c_void_p * 1)(Wp.data_ptr())
    us = C.c_float(0.0)
    Y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    assert L.t5g_time_gemm(C.c_void_p(X.data_ptr()), K, M, arr, 1, N, K, 1, C.c_void_p(Y.data_ptr()), N, 0, ITERS,
                           st, C.byref(us)) == 0
    assert math.isfinite(us.value) and us.value > 0, us.value
    Yf = torch.zeros(M, N, dtype=torch.float32, device="cuda")
    a = _lib.GemvArgs()
    a.M, a.K, a.N, a.epi, a.pro, a.nw, a.splits = M, K, N, 4, 0, 4, 1
    a.W, a.Y, a.ldy, a.X, a.ldx = Wp.data_ptr(), Yf.data_ptr(), N, X.data_ptr(), K
    us.value = 0.0
    assert L.t5g_time_gemv(C.byref(a), arr, 1, ITERS, st, C.byref(us)) == 0
    assert math.isfinite(us.value) and us.value > 0, us.value
    torch.cuda.synchronize()
    # both timed the same Linear
    assert torch.allclose(Y.float(), Yf, rtol=2 ** -7, atol=1e-6)

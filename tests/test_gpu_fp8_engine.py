"""FP8 e4m3 decode weights, engine level (weight_format="fp8"): the contract of DESIGN.md §5
"FP8 mode" -- an FP8 engine's fast path is, bit for bit, the bf16 fast path on the rounded
weights W_q -- held without a tolerance on the golden_mid config (true 2b-2b widths, 2 + 2
layers), plus what the mode refuses. FP8 engines run the per-op launches at every batch size;
the bf16 engine they are compared with runs its default launches."""
import pytest
import torch

from tests.engine_cases import assert_same_run, both_loops, default_params, mid_config, need_gpu, utterances

pytestmark = pytest.mark.gpu

_STATE = {}


def _setup():
    """cfg, sd, the FP8 engine (A) and the bf16 engine on fp8_rounded_state_dict (B), once."""
    if not _STATE:
        from t5gemma_tts_amd.engine import T5GemmaTTSEngine
        from t5gemma_tts_amd.weights import fp8_rounded_state_dict
        cfg, sd = mid_config()
        kw = dict(device="cuda:0", max_batch=20, max_text=64, max_audio=128, max_gen=40)
        _STATE["cfg"], _STATE["sd"], _STATE["kw"] = cfg, sd, kw
        _STATE["A"] = T5GemmaTTSEngine(cfg, sd, weight_format="fp8", **kw)
        _STATE["B"] = T5GemmaTTSEngine(cfg, fp8_rounded_state_dict(cfg, sd), **kw)
    return _STATE


def _both_loops(eng, utts, seeds):
    """(host, fast) of engine_cases.both_loops, the on-device graph loop run first."""
    return both_loops(eng, utts, seeds, host_first=False)


def _assert_both_same(a, b, B):
    (ha, fa), (hb, fb) = a, b
    assert_same_run(fa, fb, B, "graph")
    assert_same_run(ha, hb, B, "host")
    assert len(ha["logits"]) > 1
    assert sum(len(g) for g in fa["gen"]) > B


@pytest.mark.parametrize("B,fused", [(1, True), (8, True), (16, True), (8, False), (20, False)])
def test_fp8_engine_is_bitwise_the_bf16_fast_path_on_rounded_weights(B, fused):
    need_gpu()
    st = _setup()
    utts = utterances(st["cfg"], B, 90 + B)
    seeds = list(range(700, 700 + B))
    try:
        st["A"].set_fused(fused)
        st["B"].set_fused(fused)
        launches = st["A"].block_launches()
        _assert_both_same(_both_loops(st["A"], utts, seeds), _both_loops(st["B"], utts, seeds), B)
        assert st["A"].block_launches() == launches   # FP8 mode: per-op launches only
    finally:
        st["A"].set_fused(True)
        st["B"].set_fused(True)


def test_fp8_engine_is_not_bf16_in_disguise():
    need_gpu()
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    st = _setup()
    assert st["A"].native_weight_format() == "fp8" and st["B"].native_weight_format() == "bf16"
    utts = utterances(st["cfg"], 8, 31)
    seeds = list(range(40, 48))
    a = st["A"].generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True)
    raw = T5GemmaTTSEngine(st["cfg"], st["sd"], shared_from=None, **st["kw"])
    try:
        r = raw.generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True)
    finally:
        raw.close()
    la, lr = a["logits"][0], r["logits"][0]
    assert bool(torch.isfinite(la.float()).all())
    assert not torch.equal(la.view(torch.int16), lr.view(torch.int16))


def test_fp8_handoff_poison_reruns_on_per_op_launches():
    """As test_handoff_timeout_falls_back_to_per_op_launches, on an FP8 engine: the sticky
    timeout word makes t5g_read_tokens report T5G_EHANDOFF, engine.generate reruns the call
    with set_fused(False) -- the same tokens -- and the next call is clean again."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    st = _setup()
    eng = st["A"]
    utts = utterances(st["cfg"], 8, 77)
    seeds = list(range(500, 508))
    ref = eng.generate(utts, default_params(), seeds=seeds)
    _lib.check(_lib.lib().t5g_engine_poison_handoff(eng.h, 99), "poison_handoff")
    with pytest.warns(UserWarning):
        out = eng.generate(utts, default_params(), seeds=seeds)
    again = eng.generate(utts, default_params(), seeds=seeds)
    for b in range(8):
        assert out["gen"][b].tolist() == ref["gen"][b].tolist(), b
        assert again["gen"][b].tolist() == ref["gen"][b].tolist(), b


def test_fp8_refusals():
    need_gpu()
    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import synthetic_weights
    st = _setup()
    utts = utterances(st["cfg"], 1, 5)
    with pytest.raises(ValueError):
        st["A"].generate(utts, default_params(), seeds=[1], parity=True)
    with pytest.raises(ValueError):
        st["A"].set_exact(True)
    assert _lib.lib().t5g_engine_set_exact(st["A"].h, 1, _lib.gelu_erf_table(), _lib.EXACT_THREADS) \
        == _lib.T5G_EUNSUPPORTED
    tiny = named_config("tiny")
    with pytest.raises(ValueError):
        T5GemmaTTSEngine(tiny, synthetic_weights(tiny, 7), device="cuda:0", max_batch=1, max_text=32,
                         max_audio=64, weight_format="fp8")
    for owner, fmt in ((st["A"], "bf16"), (st["B"], "fp8")):
        with pytest.raises(ValueError):
            T5GemmaTTSEngine(st["cfg"], {}, shared_from=owner, weight_format=fmt, **st["kw"])
    # a second arena on the FP8 engine's weights computes what the first does
    twin = T5GemmaTTSEngine(st["cfg"], {}, shared_from=st["A"], weight_format="fp8", **st["kw"])
    try:
        assert twin.native_weight_format() == "fp8"
        a = st["A"].generate(utts, default_params(), seeds=[9])
        b = twin.generate(utts, default_params(), seeds=[9])
        assert a["gen"][0].tolist() == b["gen"][0].tolist()
    finally:
        twin.close()
    # the native call itself refuses the widths it has no kernels for
    teng = T5GemmaTTSEngine(tiny, synthetic_weights(tiny, 7), device="cuda:0", max_batch=1, max_text=32, max_audio=64)
    try:
        w8 = _lib.Fp8Weights()
        assert _lib.lib().t5g_engine_set_fp8_weights(teng.h, w8) == _lib.T5G_EUNSUPPORTED
    finally:
        teng.close()

"""FP8 weights in the persistent MLP-half launch (csrc/fused_mlp_p8.hip: fused_mlp_kernel<9> at
1-16 decode rows, <10> at 17-32, on the P8 code images of gate/up and down, behind set_fp8_mlp,
off by default). The contract of DESIGN.md §5 "FP8 mode" without a tolerance: an FP8 engine with
the switch on computes, bit for bit, what it computes on the per-op P8 launches and what a bf16
engine on the rounded weights W_q computes on its default launches. golden_mid at the true 2b-2b
widths with 2 + 2 layers: the smallest model the launch accepts. Row counts: one live row of a
tile (1), a full tile (16), a second tile with one live row (17: the min(row, M - 1) clamp and
the zeroed fragments), a ragged second tile (20), both tiles full (32). Reference: PMDecoderLayer's
cross-attention residual + T5GemmaMLP, hf_export/modeling_t5gemma_voice.py:256-323 (what every
layout computes)."""
import ctypes as C
import functools
import warnings

import pytest

from tests.engine_cases import assert_same_run, default_params, mid_config, need_gpu, stream, utterances

pytestmark = pytest.mark.gpu

# ragged rows as engine_cases.utterances makes them; row 0 has no prompt, row 1 has 64 text keys,
# row 2 has 4
ROWS = dict(bare_first=True, text_lens={1: 64, 2: 4})
KW = dict(device="cuda:0", max_text=64, max_gen=40, max_audio=128, max_batch=32)


@functools.lru_cache(maxsize=None)
def _fp8_engine(fp8_mlp=False):
    """The 32-row FP8 engine (A); the first one quantises, the other is a twin on its weights
    built with the keyword (the switch is launch state: every twin has its own)."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    cfg, sd = mid_config()
    if not fp8_mlp:
        return T5GemmaTTSEngine(cfg, sd, weight_format="fp8", **KW)
    return T5GemmaTTSEngine(cfg, {}, shared_from=_fp8_engine(), weight_format="fp8", fp8_mlp=True, **KW)


@functools.lru_cache(maxsize=None)
def _bf16_engine():
    """The 32-row bf16 engine (B) on the rounded weights."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import fp8_rounded_state_dict
    cfg, sd = mid_config()
    return T5GemmaTTSEngine(cfg, fp8_rounded_state_dict(cfg, sd), **KW)


def _run(eng, utts, seeds):
    """Host loop (every step's logits) and the graph-replayed on-device loop (tokens), with the
    MLP-half and whole-layer launches each issued. Warnings are errors: a hand-off that gave up
    would rerun the call on the per-op launches (the same tokens) -- here that is a failure of
    the launch under test, not a fallback to accept."""
    m0, b0 = eng.mlp_half_launches(), eng.block_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host = eng.generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True)
        fast = eng.generate(utts, default_params(), seeds=seeds)
    return host, fast, eng.mlp_half_launches() - m0, eng.block_launches() - b0


def _same(a, b, B, tag):
    assert_same_run(a[0], b[0], B, ("host", tag))
    assert_same_run(a[1], b[1], B, ("graph", tag))


@pytest.mark.parametrize("B", [1, 8, 16, 17, 20, 32])
def test_fp8_mlp_is_bitwise_the_per_op_p8_and_the_bf16_launches(B):
    need_gpu()
    cfg, _ = mid_config()
    A, Bf = _fp8_engine(), _bf16_engine()
    utts = utterances(cfg, B, 410 + B, **ROWS)
    seeds = list(range(700, 700 + B))
    L = cfg.backbone.num_decoder_layers
    try:
        A.set_fp8_mlp(True)
        on = _run(A, utts, seeds)
        A.set_fp8_mlp(False)
        off = _run(A, utts, seeds)
    finally:
        A.set_fp8_mlp(False)
    ref = _run(Bf, utts, seeds)
    _same(on, off, B, "per-op P8")
    _same(on, ref, B, "bf16 on W_q")
    # the P8 MLP-half launch ran with the switch on (one per layer and captured step at least)
    # and not with it off; no whole-layer launch either way
    assert on[2] >= L and off[2] == 0, (on[2], off[2])
    assert on[3] == 0 and off[3] == 0, (on[3], off[3])
    assert len(on[0]["logits"]) > 1
    assert sum(len(g) for g in on[0]["gen"]) > B


def test_fp8_mlp_with_fp8_block():
    """Both switches on: 16 rows take the P8 whole-layer launch, 17 rows the P8 MLP-half."""
    need_gpu()
    cfg, _ = mid_config()
    A = _fp8_engine()
    L = cfg.backbone.num_decoder_layers
    utts = utterances(cfg, 17, 433, **ROWS)
    seeds = list(range(17))
    try:
        A.set_fp8_mlp(True)
        A.set_fp8_block(True)
        on16 = _run(A, utts[:16], seeds[:16])
        on17 = _run(A, utts, seeds)
        A.set_fp8_mlp(False)
        A.set_fp8_block(False)
        off16 = _run(A, utts[:16], seeds[:16])
        off17 = _run(A, utts, seeds)
    finally:
        A.set_fp8_mlp(False)
        A.set_fp8_block(False)
    assert on16[3] >= L and on16[2] == 0, on16[2:]
    assert on17[2] >= L and on17[3] == 0, on17[2:]
    assert off16[2:] == (0, 0) and off17[2:] == (0, 0), (off16[2:], off17[2:])
    _same(on16, off16, 16, "16 rows")
    _same(on17, off17, 17, "17 rows")


def test_fp8_mlp_set_fused_off_runs_per_op():
    need_gpu()
    cfg, _ = mid_config()
    A = _fp8_engine()
    utts = utterances(cfg, 20, 447, **ROWS)
    seeds = list(range(20))
    try:
        A.set_fp8_mlp(True)
        on = _run(A, utts, seeds)
        A.set_fused(False)
        unfused = _run(A, utts, seeds)
    finally:
        A.set_fused(True)
        A.set_fp8_mlp(False)
    assert on[2] >= cfg.backbone.num_decoder_layers and unfused[2] == 0, (on[2], unfused[2])
    _same(on, unfused, 20, "set_fused(False)")


def test_fp8_mlp_repeated_calls():
    """The same 32-row call twice: the hand-off counters reset themselves."""
    need_gpu()
    cfg, _ = mid_config()
    A = _fp8_engine()
    utts = utterances(cfg, 32, 461, **ROWS)
    seeds = list(range(32))
    try:
        A.set_fp8_mlp(True)
        one = _run(A, utts, seeds)
        two = _run(A, utts, seeds)
    finally:
        A.set_fp8_mlp(False)
    L = cfg.backbone.num_decoder_layers
    assert one[2] >= L and two[2] >= L, (one[2], two[2])
    _same(one, two, 32, "repeat")


def test_fp8_mlp_rows_are_independent():
    """Rows 0, 16 and 31 of a 32-row call (fused_mlp_kernel<10>) give the tokens of the same
    utterances run alone (<9>): the two tiles and the two kernels agree."""
    need_gpu()
    cfg, _ = mid_config()
    A = _fp8_engine()
    utts = utterances(cfg, 32, 93, **ROWS)
    seeds = list(range(60, 92))
    L = cfg.backbone.num_decoder_layers
    try:
        A.set_fp8_mlp(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # no rerun on the per-op launches (see _run)
            m0 = A.mlp_half_launches()
            full = A.generate(utts, default_params(), seeds=seeds)
            assert A.mlp_half_launches() - m0 >= L
            for r in (0, 16, 31):
                m0 = A.mlp_half_launches()
                alone = A.generate([utts[r]], default_params(), seeds=[seeds[r]])
                assert A.mlp_half_launches() - m0 >= L
                assert alone["gen"][0].tolist() == full["gen"][r].tolist(), r
    finally:
        A.set_fp8_mlp(False)


def test_fp8_mlp_handoff_poison_reruns_on_per_op_launches():
    """The sticky timeout word makes t5g_read_tokens report T5G_EHANDOFF on the P8 MLP-half
    launch; engine.generate reruns the call with set_fused(False) -- the per-op P8 launches, the
    same tokens -- and the next call is clean again. The one place a warning is expected."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    cfg, _ = mid_config()
    A = _fp8_engine()
    utts = utterances(cfg, 32, 79, **ROWS)
    seeds = list(range(520, 552))
    try:
        A.set_fp8_mlp(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m0 = A.mlp_half_launches()
            ref = A.generate(utts, default_params(), seeds=seeds)
            assert A.mlp_half_launches() > m0
        _lib.check(_lib.lib().t5g_engine_poison_handoff(A.h, 99), "poison_handoff")
        with pytest.warns(UserWarning):
            out = A.generate(utts, default_params(), seeds=seeds)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            m1 = A.mlp_half_launches()
            again = A.generate(utts, default_params(), seeds=seeds)
            assert A.mlp_half_launches() > m1   # back on the P8 MLP-half launch
    finally:
        A.set_fp8_mlp(False)
    for b in range(32):
        assert out["gen"][b].tolist() == ref["gen"][b].tolist(), b
        assert again["gen"][b].tolist() == ref["gen"][b].tolist(), b


def test_fp8_mlp_switch_semantics():
    need_gpu()
    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    cfg, sd = mid_config()
    L = _lib.lib()
    # a bf16 engine has no such launch
    Bf = _bf16_engine()
    with pytest.raises(ValueError):
        Bf.set_fp8_mlp(True)
    assert L.t5g_engine_set_fp8_mlp(Bf.h, 1) == _lib.T5G_EUNSUPPORTED
    assert L.t5g_engine_set_fp8_mlp(Bf.h, 0) == 0
    with pytest.raises(ValueError):
        T5GemmaTTSEngine(cfg, {}, shared_from=Bf, fp8_mlp=True, **KW)
    # the constructor keyword reaches the native engine: a twin built with it takes the launch
    on = _fp8_engine(True)
    utts = utterances(cfg, 32, 157, **ROWS)
    seeds = list(range(32))
    m0 = on.mlp_half_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        first = on.generate(utts, default_params(), seeds=seeds)
    assert on.mlp_half_launches() - m0 >= cfg.backbone.num_decoder_layers
    # the timing hook serves an FP8 engine exactly when the switch is on (state after a call);
    # the engine the twin shares its weights with keeps its own switch (off)
    us = C.c_float()
    st = stream()
    assert L.t5g_time_decode_mlp(_fp8_engine().h, 32, 4, st, C.byref(us)) == _lib.T5G_EUNSUPPORTED
    assert L.t5g_time_decode_mlp(on.h, 32, 4, st, C.byref(us)) == 0
    assert us.value > 0
    on.set_fp8_mlp(False)
    try:
        assert L.t5g_time_decode_mlp(on.h, 32, 4, st, C.byref(us)) == _lib.T5G_EUNSUPPORTED
    finally:
        on.set_fp8_mlp(True)
    # a fresh generate after the hook succeeds, on the launch, with the same tokens
    m1 = on.mlp_half_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        after = on.generate(utts, default_params(), seeds=seeds)
    assert on.mlp_half_launches() > m1
    for b in range(32):
        assert after["gen"][b].tolist() == first["gen"][b].tolist(), b

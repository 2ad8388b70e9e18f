"""FP8 weights in the whole-layer persistent launch (csrc/fused_p8.hip: fused_block_kernel on
P8 code images, 1-16 decode rows, behind set_fp8_block, off by default). The contract of
DESIGN.md §5 "FP8 mode" without a tolerance: an FP8 engine with the switch on computes, bit for
bit, what it computes on the per-op P8 launches and what a bf16 engine on the rounded weights
W_q computes on its default launches. golden_mid at the true 2b-2b widths with 2 + 2 layers: the
smallest model the launch accepts, with one launch that carries the next layer's q|k|v and
o-projection weights and a last launch that does not. Stage S placements by the slot rules of
DESIGN.md §4.5 (256 workgroups, 4 kv heads, M rows, n 64-key chunks of the call's key bound):
the tail takes M * 4 * n <= 2 * (256 - M) slots, the front 768 per pass and two passes, past
that S runs as its own launch. Reference: PMDecoderLayer,
hf_export/modeling_t5gemma_voice.py:256-323 (what every layout computes)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

from tests.engine_cases import assert_same_run, default_params, mid_config, need_gpu, stream, utterances

pytestmark = pytest.mark.gpu

# ragged rows as engine_cases.utterances makes them; row 0 has no prompt, row 1 has 64 text keys
# (the most the launch's cross attention reads), row 2 has 4
ROWS = dict(bare_first=True, text_lens={1: 64, 2: 4})
KW = dict(device="cuda:0", max_text=64, max_gen=40)


@functools.lru_cache(maxsize=None)
def _fp8_engine(max_audio, max_batch=16, fp8_block=False):
    """The FP8 engine (A) of one cache size; the first one quantises, the others are twins on
    its weights (the switch is launch state: every twin has its own)."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    cfg, sd = mid_config()
    kw = dict(KW, max_batch=max_batch, max_audio=max_audio, weight_format="fp8", fp8_block=fp8_block)
    if (max_audio, max_batch, fp8_block) == (128, 16, False):
        return T5GemmaTTSEngine(cfg, sd, **kw)
    return T5GemmaTTSEngine(cfg, {}, shared_from=_fp8_engine(128), **kw)


@functools.lru_cache(maxsize=None)
def _bf16_engine():
    """The bf16 engine (B) on the rounded weights."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import fp8_rounded_state_dict
    cfg, sd = mid_config()
    return T5GemmaTTSEngine(cfg, fp8_rounded_state_dict(cfg, sd), max_batch=16, max_audio=128, **KW)


def _run(eng, utts, seeds):
    """Host loop (every step's logits) and the graph-replayed on-device loop (tokens), with the
    whole-layer and stage S launches each issued. Warnings are errors: a hand-off that gave up
    would rerun the call on the per-op launches (the same tokens) -- here that is a failure of
    the launch under test, not a fallback to accept."""
    b0, s0 = eng.block_launches(), eng.attn_in_block_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host = eng.generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True)
        mode = eng.attn_in_block_mode()
        fast = eng.generate(utts, default_params(), seeds=seeds)
    return host, fast, eng.block_launches() - b0, eng.attn_in_block_launches() - s0, mode


def _with_long_row(cfg, utts, row, max_audio):
    """Row `row` with an explicit prompt of max_audio - 44 codes: prompt + budget + 1 then lies
    in (max_audio - 64, max_audio) whatever the row's budget (9 .. 40 steps), so the call's key
    bound is max_audio and its rows have max_audio / 64 chunk slots each."""
    from t5gemma_tts_amd.engine import Utterance
    rng = np.random.default_rng(max_audio)
    tp = max_audio - 44
    y = rng.integers(0, 65536, size=tp).tolist() + [cfg.y_sep_token]
    out = list(utts)
    out[row] = Utterance(x=utts[row].x, y=y, tgt_y_len=len(y) + 12)
    return out


@pytest.mark.parametrize("B", [1, 3, 8, 16])
def test_fp8_block_is_bitwise_the_per_op_p8_and_the_bf16_launches(B):
    need_gpu()
    cfg, _ = mid_config()
    A, Bf = _fp8_engine(128), _bf16_engine()
    utts = utterances(cfg, B, 310 + B, **ROWS)
    seeds = list(range(900, 900 + B))
    L = cfg.backbone.num_decoder_layers
    try:
        A.set_fp8_block(True)
        on = _run(A, utts, seeds)
        A.set_fp8_block(False)
        off = _run(A, utts, seeds)
    finally:
        A.set_fp8_block(False)
    ref = _run(Bf, utts, seeds)
    for tag, other in (("per-op P8", off), ("bf16 on W_q", ref)):
        assert_same_run(on[0], other[0], B, ("host", tag))
        assert_same_run(on[1], other[1], B, ("graph", tag))
    # the P8 whole-layer launch ran with the switch on (one per layer and captured step at
    # least) and not with it off
    assert on[2] >= L and off[2] == 0, (on[2], off[2])
    assert len(on[0]["logits"]) > 1
    assert sum(len(g) for g in on[0]["gen"]) > B


@pytest.mark.parametrize("B,max_audio,mode,expect", [
    (8, 128, 2, 2), (16, 128, 2, 2),   # 2 chunks: 64 / 128 slots <= 2 per worker -- the tail
    (8, 128, 1, 1),                    # the same call with S in front
    (16, 512, 2, 1),                   # 8 chunks: 512 slots > 480 tail slots -- in front, one pass
    (16, 896, 1, 1),                   # 14 chunks: 896 slots > 768 -- two passes
    (16, 1664, 2, 0),                  # 26 chunks: 1 664 slots > 1 536 -- S as its own launch, the P8 block still running
])
def test_fp8_block_attention_in_block(B, max_audio, mode, expect):
    need_gpu()
    cfg, _ = mid_config()
    # the table's placements by the slot rules, before anything runs
    slots, nw = B * 4 * (max_audio // 64), 256 - B
    want = 2 if mode == 2 and slots <= 2 * nw else 1 if slots <= 2 * 768 else 0
    assert want == expect, (slots, nw)
    eng = _fp8_engine(max_audio)
    utts = _with_long_row(cfg, utterances(cfg, B, 50 + B + max_audio, **ROWS), 3, max_audio)
    seeds = list(range(B))
    L = cfg.backbone.num_decoder_layers
    try:
        eng.set_fp8_block(True)
        eng.set_attn_in_block(mode)
        on, fon, nb_on, ns_on, m_on = _run(eng, utts, seeds)
        eng.set_attn_in_block(0)
        off, foff, nb_off, ns_off, m_off = _run(eng, utts, seeds)
    finally:
        eng.set_attn_in_block(2)
        eng.set_fp8_block(False)
    assert m_on == expect and m_off == 0, (m_on, m_off)
    assert (ns_on > 0) == (expect != 0) and ns_off == 0, (ns_on, ns_off)   # S ran exactly where expected
    assert nb_on >= L and nb_off >= L, (nb_on, nb_off)                     # the P8 block ran either way
    assert_same_run(on, off, B, "on/off")
    assert_same_run(fon, foff, B, "graph on/off")
    assert sum(len(g) for g in on["gen"]) > B


def test_fp8_block_rows_are_independent():
    """Rows 0 and 15 of a 16-row call give the tokens of the same utterances run alone."""
    need_gpu()
    cfg, _ = mid_config()
    eng = _fp8_engine(128)
    utts = utterances(cfg, 16, 93, **ROWS)
    seeds = list(range(60, 76))
    try:
        eng.set_fp8_block(True)
        b0 = eng.block_launches()
        with warnings.catch_warnings():
            warnings.simplefilter("error")   # no rerun on the per-op launches (see _run)
            full = eng.generate(utts, default_params(), seeds=seeds)
            assert eng.block_launches() - b0 >= cfg.backbone.num_decoder_layers
            for r in (0, 15):
                alone = eng.generate([utts[r]], default_params(), seeds=[seeds[r]])
                assert alone["gen"][0].tolist() == full["gen"][r].tolist(), r
    finally:
        eng.set_fp8_block(False)


def test_fp8_block_handoff_poison_reruns_on_per_op_launches():
    """The sticky timeout word makes t5g_read_tokens report T5G_EHANDOFF on the P8 block;
    engine.generate reruns the call with set_fused(False) -- for an FP8 engine the per-op P8
    launches, the same tokens -- and the next call is clean again. The one place a warning is
    expected."""
    need_gpu()
    from t5gemma_tts_amd import _lib
    cfg, _ = mid_config()
    eng = _fp8_engine(128)
    utts = utterances(cfg, 8, 79, **ROWS)
    seeds = list(range(520, 528))
    try:
        eng.set_fp8_block(True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            b0 = eng.block_launches()
            ref = eng.generate(utts, default_params(), seeds=seeds)
            assert eng.block_launches() > b0
        _lib.check(_lib.lib().t5g_engine_poison_handoff(eng.h, 99), "poison_handoff")
        with pytest.warns(UserWarning):
            out = eng.generate(utts, default_params(), seeds=seeds)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            b1 = eng.block_launches()
            again = eng.generate(utts, default_params(), seeds=seeds)
            assert eng.block_launches() > b1   # back on the P8 block
    finally:
        eng.set_fp8_block(False)
    for b in range(8):
        assert out["gen"][b].tolist() == ref["gen"][b].tolist(), b
        assert again["gen"][b].tolist() == ref["gen"][b].tolist(), b


def test_fp8_block_switch_semantics():
    need_gpu()
    from t5gemma_tts_amd import _lib
    cfg, _ = mid_config()
    L = _lib.lib()
    # a bf16 engine has no such launch
    Bf = _bf16_engine()
    with pytest.raises(ValueError):
        Bf.set_fp8_block(True)
    assert L.t5g_engine_set_fp8_block(Bf.h, 1) == _lib.T5G_EUNSUPPORTED
    assert L.t5g_engine_set_fp8_block(Bf.h, 0) == 0
    # 17 rows stay on the per-op P8 launches with the switch on (a twin built with the keyword)
    big = _fp8_engine(128, 17, True)
    utts = utterances(cfg, 17, 157, **ROWS)
    seeds = list(range(17))
    big.set_block_max_rows(32)   # the bf16 engine's two-tile limit does not apply to FP8
    try:
        on = _run(big, utts, seeds)
        big.set_fp8_block(False)
        off = _run(big, utts, seeds)
    finally:
        big.set_block_max_rows(16)
        big.set_fp8_block(True)
    assert on[2] == 0 and off[2] == 0, (on[2], off[2])
    assert_same_run(on[0], off[0], 17, "host 17")
    assert_same_run(on[1], off[1], 17, "graph 17")
    # ... and 16 rows of the same twin take the block: the keyword reached the native engine
    b0 = big.block_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        big.generate(utts[:16], default_params(), seeds=seeds[:16])
    assert big.block_launches() - b0 >= cfg.backbone.num_decoder_layers
    # the timing hook serves an FP8 engine exactly when the switch is on (state after a call)
    us, keys = C.c_float(), C.c_float()
    st = stream()
    assert L.t5g_time_decode_layer(big.h, 16, 4, st, C.byref(us), C.byref(keys)) == 0
    assert us.value > 0
    big.set_fp8_block(False)
    try:
        assert L.t5g_time_decode_layer(big.h, 16, 4, st, C.byref(us), C.byref(keys)) == _lib.T5G_EUNSUPPORTED
        assert L.t5g_time_decode_mlp(big.h, 16, 4, st, C.byref(us)) == _lib.T5G_EUNSUPPORTED
    finally:
        big.set_fp8_block(True)

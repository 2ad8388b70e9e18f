"""The whole-layer persistent launch at 17-32 rows (csrc/fused_kernels.h fused_block_kernel with two
16-row MFMA tiles per GEMV stage, compiled in csrc/fused_rows32.hip; a norm workgroup per two
rows, a cross-attention workgroup per (row, kv head)), enabled by set_block_max_rows(32),
against the same step on the per-op launches: tokens and every logit row bitwise equal at the
true 2b-2b widths (2 + 2 layers). Sizes: 17 (one live row in the second tile), 20, 25 and 26
(the first sizes at which one norm workgroup per row would leave the down / gate-up stages 6
units per worker), 32 (full). Stage S (the decode self attention inside the launch) at 20 and
32 rows in the tail, in front in one and in two passes, and past two passes (its own launch,
the block still running). Rows of a 32-row call give the tokens of the same utterances run
alone. Reference: PMDecoderLayer, hf_export/modeling_t5gemma_voice.py:256-323, and
T5GemmaMLP, [tf] modeling_t5gemma.py:81-97 (what both layouts compute)."""
import functools
import os
import re

import pytest

from conftest import REPO
from tests.engine_cases import assert_same_run, default_params, mid_engine, need_gpu, utterances

gpu = pytest.mark.gpu

# ragged rows as engine_cases.utterances makes them; row 0 has no prompt, row 1 has 64 text keys
# (the most the launch's cross attention reads), row 2 has 4
ROWS = dict(bare_first=True, text_lens={1: 64, 2: 4})


@functools.lru_cache(maxsize=None)
def _engine(max_audio):
    """engine_cases.mid_engine(32, max_audio) (golden_mid at the true widths, 2 + 2 layers,
    max_text 64), shared by the tests of one cache size."""
    return mid_engine(32, max_audio)


def _run(eng, utts, seeds):
    """Host loop (every step's logits) and the graph-replayed on-device loop (tokens), with the
    whole-layer and stage S launches each issued."""
    import warnings
    b0, s0 = eng.block_launches(), eng.attn_in_block_launches()
    with warnings.catch_warnings():
        # a hand-off that gave up would rerun the call on the per-op launches (the same
        # tokens): here that is a failure of the launch under test, not a fallback to accept
        warnings.simplefilter("error")
        # not engine_cases.both_loops: the placement is read between the two loops
        host = eng.generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True)
        mode = eng.attn_in_block_mode()
        fast = eng.generate(utts, default_params(), seeds=seeds)
    return host, fast, eng.block_launches() - b0, eng.attn_in_block_launches() - s0, mode


@gpu
@pytest.mark.parametrize("B", [17, 20, 25, 26, 32])
def test_block_rows32_bitwise_equal_to_per_op_launches(B):
    need_gpu()
    cfg, eng = _engine(128)
    eng.set_block_max_rows(32)
    eng.set_attn_in_block(2)
    utts = utterances(cfg, B, 140 + B, **ROWS)
    seeds = list(range(700, 700 + B))
    L = cfg.backbone.num_decoder_layers
    runs = []
    try:
        for fused in (True, False, True):
            eng.set_fused(fused)
            runs.append(_run(eng, utts, seeds))
    finally:
        eng.set_fused(True)
    for k in (1, 2):
        assert_same_run(runs[0][0], runs[k][0], B, ("host", k))
        assert_same_run(runs[0][1], runs[k][1], B, ("graph", k))
    # the whole-layer launch ran in the fused runs (one per layer and captured step at least)
    # and not in the per-op run
    assert runs[0][2] >= L and runs[2][2] >= L and runs[1][2] == 0, [r[2] for r in runs]
    assert sum(len(g) for g in runs[0][0]["gen"]) > B


@gpu
@pytest.mark.parametrize("B,max_audio,mode,expect", [
    (20, 128, 2, 2), (32, 128, 2, 2),     # key bound 128: 2 chunks, <= 2 slots per worker -- the tail
    (20, 128, 1, 1), (32, 128, 1, 1),     # the same calls with S in front
    (32, 384, 2, 1), (32, 384, 1, 1),     # 6 chunks: 768 slots > 2 per worker; in front, one pass of 3 per workgroup
    (32, 640, 2, 1), (20, 640, 1, 1),     # 10 chunks: 1 280 / 800 slots, two passes
    (32, 960, 2, 0),                      # 15 chunks: 1 920 slots > 1 536 -- S as its own launch
])
def test_block_rows32_attention_in_block(B, max_audio, mode, expect):
    need_gpu()
    cfg, eng = _engine(max_audio)
    eng.set_block_max_rows(32)
    eng.set_fused(True)
    utts = utterances(cfg, B, 30 + B + max_audio, tp_max=max_audio - 45, **ROWS)
    seeds = list(range(B))
    L = cfg.backbone.num_decoder_layers
    try:
        eng.set_attn_in_block(mode)
        on, fon, nb_on, ns_on, m_on = _run(eng, utts, seeds)
        eng.set_attn_in_block(0)
        off, foff, nb_off, ns_off, m_off = _run(eng, utts, seeds)
    finally:
        eng.set_attn_in_block(2)
    assert m_on == expect and m_off == 0, (m_on, m_off)
    assert (ns_on > 0) == (expect != 0) and ns_off == 0, (ns_on, ns_off)   # S ran exactly where expected
    assert nb_on >= L and nb_off >= L, (nb_on, nb_off)                     # the whole-layer launch ran either way
    assert_same_run(on, off, B, "on/off")
    assert_same_run(fon, foff, B, "graph on/off")
    assert sum(len(g) for g in on["gen"]) > B


@gpu
def test_block_rows32_rows_are_independent():
    """Rows 0, 16 and 31 of a 32-row call (the first row of each tile and the last row) give
    the tokens of the same utterances run alone with the same seeds."""
    need_gpu()
    cfg, eng = _engine(128)
    eng.set_block_max_rows(32)
    eng.set_fused(True)
    eng.set_attn_in_block(2)
    utts = utterances(cfg, 32, 91, **ROWS)
    seeds = list(range(40, 72))
    import warnings
    b0 = eng.block_launches()
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # no rerun on the per-op launches (see _run)
        full = eng.generate(utts, default_params(), seeds=seeds)
        assert eng.block_launches() - b0 >= cfg.backbone.num_decoder_layers
        for r in (0, 16, 31):
            alone = eng.generate([utts[r]], default_params(), seeds=[seeds[r]])
            assert alone["gen"][0].tolist() == full["gen"][r].tolist(), r


def test_block_rows32_interface_declared_and_exported():
    """CPU: include/t5gtts.h declares t5g_engine_block_launches and
    t5g_engine_set_block_max_rows, and libt5gtts.so exports and binds them."""
    from t5gemma_tts_amd import _lib
    src = open(os.path.join(REPO, "include", "t5gtts.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = _lib.lib()
    for name in ("t5g_engine_block_launches", "t5g_engine_set_block_max_rows"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    # argument checks need no device: a null engine and a row limit other than 16 / 32
    assert L.t5g_engine_set_block_max_rows(None, 32) < 0
    assert L.t5g_engine_block_launches(None, None) < 0

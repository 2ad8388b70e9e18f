"""The fast decode path on an eager checkpoint -- what a checkpoint loaded with its defaults is
(config.py: attn_implementation "eager", the 50.0 tanh logit softcap on) -- at the engine level:
golden_mid (2 + 2 layers at the true 2b-2b widths, max_text 64, max_gen 40) with
attn_implementation="eager", where every fast-path decode attention score goes through
csrc/common.h fast_score at its three call sites: the decode attention launches (csrc/attn.hip),
stage S of the persistent layer launch (csrc/fused_attn.h) and its in-launch cross attention,
stage A (csrc/fused_kernels.h). The sdpa tests of the persistent launches, restated on that model:

* the softcap is live: step-0 logits differ in bits from the sdpa engine's on the same call;
* the persistent launches (whole layer at 1-16 rows and, two-tile, at 17-32; the MLP half at 32
  rows) against the per-op launches, rows reading 64 and 4 text keys in stage A;
* stage S at the end of the previous launch (2), in front (1) and as its own flash launch (0),
  with rows that cross 64 keys mid-call and on a sliding layer past its 100-key window;
* FP8 weights in the whole-layer launch (3 and 16 rows) and in the MLP-half launch (20 rows)
  against the per-op FP8 launches and against a bf16 engine on the rounded weights.

Every comparison is bitwise: the tokens of the graph-replayed loop, the tokens and every step's
logits of the host loop (engine_cases.both_loops / assert_same_run), with warnings as errors so
that a hand-off that fell back to the per-op launches cannot pass as the launch under test. The
score's value is held by tests/test_gpu_attn_softcap.py at the kernel level; these tests hold the
three sites to one another. Reference: [tf] eager_attention_forward, modeling_t5gemma.py:199-230,
inside PMDecoderLayer, hf_export/modeling_t5gemma_voice.py:256-323."""
import functools
import warnings

import numpy as np
import pytest
import torch

from tests.engine_cases import (assert_same_run, both_loops, default_params, mid_config, mid_engine, need_gpu,
                                utterances)

pytestmark = pytest.mark.gpu

# ragged rows as engine_cases.utterances makes them; row 0 has no prompt, row 1 has 64 text keys
# (the most the launch's cross attention reads), row 2 has 4
ROWS = dict(bare_first=True, text_lens={1: 64, 2: 4})
KW = dict(device="cuda:0", max_text=64, max_gen=40, max_audio=128, max_batch=32)


@functools.lru_cache(maxsize=None)
def _eager(max_audio=128, window=None):
    """(cfg, the eager bf16 engine) of one cache size / window, made once."""
    cfg, eng = mid_engine(32 if window is None else 8, max_audio, window=window, attn_implementation="eager")
    assert cfg.backbone.softcap == 50.0
    return cfg, eng


@functools.lru_cache(maxsize=None)
def _fp8_pair():
    """(the eager FP8 engine, the eager bf16 engine on its rounded weights W_q)."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import fp8_rounded_state_dict
    cfg, sd = mid_config(attn_implementation="eager")
    return (T5GemmaTTSEngine(cfg, sd, weight_format="fp8", **KW),
            T5GemmaTTSEngine(cfg, fp8_rounded_state_dict(cfg, sd), **KW))


def _run(eng, utts, seeds):
    """both_loops with warnings as errors, and the launch counters' rise: (host, graph, whole-layer
    launches, MLP-half launches, launches with stage S inside)."""
    n0 = (eng.block_launches(), eng.mlp_half_launches(), eng.attn_in_block_launches())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        host, fast = both_loops(eng, utts, seeds)
    return host, fast, eng.block_launches() - n0[0], eng.mlp_half_launches() - n0[1], eng.attn_in_block_launches() - n0[2]


def _same(a, b, B, tag):
    assert_same_run(a[0], b[0], B, ("host", tag))
    assert_same_run(a[1], b[1], B, ("graph", tag))


def test_softcap_is_live():
    """The same utterances and seeds on the eager and on the sdpa engine: step-0 logits differ in
    bits on every row (without this the equalities below could hold on an engine that never saw
    the softcap)."""
    need_gpu()
    cfg, eng = _eager()
    scfg, sdpa = mid_engine(8)
    assert scfg.backbone.softcap == 0.0
    B = 3
    utts = utterances(cfg, B, 41, **ROWS)
    seeds = [5, 6, 7]
    outs = []
    for e in (eng, sdpa):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            outs.append(e.generate(utts, default_params(), seeds=seeds, parity=True, exact=False, record_logits=True))
    la, lb = outs[0]["logits"][0].cpu(), outs[1]["logits"][0].cpu()
    for r in range(B):
        assert not torch.equal(la[r].view(torch.int16), lb[r].view(torch.int16)), r
        assert bool(torch.isfinite(la[r].float()).all())


@pytest.mark.parametrize("B", [1, 8, 16, 17, 32])
def test_persistent_launches_equal_per_op_launches(B):
    """set_fused(True) against set_fused(False): the whole-layer launch (17 and 32 rows: its
    two-tile form, set_block_max_rows(32)) with stages S and A inside against the flash launch,
    the per-op cross attention and the per-op GEMVs. At 32 rows also with the row limit back at
    16: the MLP-half launch."""
    need_gpu()
    cfg, eng = _eager()
    L = cfg.backbone.num_decoder_layers
    utts = utterances(cfg, B, 240 + B, **ROWS)
    seeds = list(range(300, 300 + B))
    try:
        eng.set_block_max_rows(32)
        eng.set_fused(True)
        on = _run(eng, utts, seeds)
        eng.set_fused(False)
        off = _run(eng, utts, seeds)
        _same(on, off, B, "fused / per-op")
        assert on[2] >= L and off[2] == 0 and off[3] == 0, (on[2:], off[2:])
        assert on[4] > 0 and off[4] == 0, (on[4], off[4])   # stage S ran inside the launch
        if B == 32:
            eng.set_block_max_rows(16)
            eng.set_fused(True)
            half = _run(eng, utts, seeds)
            _same(half, off, B, "MLP half / per-op")
            assert half[3] >= L and half[2] == 0, half[2:]
    finally:
        eng.set_block_max_rows(16)
        eng.set_fused(True)
    assert len(on[0]["logits"]) > 1 and sum(len(g) for g in on[0]["gen"]) > B


def _stage_s_placements(eng, utts, seeds, B):
    """Modes 2, 0, 1 and 2 again: pairwise bitwise equal (each against mode 0, and 2 against 2),
    stage S inside a launch in every mode but 0."""
    runs = {}
    try:
        for tag, mode in (("2", 2), ("0", 0), ("1", 1), ("2 again", 2)):
            eng.set_attn_in_block(mode)
            runs[tag] = _run(eng, utts, seeds)
    finally:
        eng.set_attn_in_block(2)
    assert runs["0"][4] == 0 and all(runs[t][4] > 0 for t in ("2", "1", "2 again")), {t: r[4] for t, r in runs.items()}
    for t in ("2", "1", "2 again"):
        _same(runs[t], runs["0"], B, f"mode {t} / 0")
    _same(runs["2"], runs["2 again"], B, "mode 2 / 2")
    _same(runs["2"], runs["1"], B, "mode 2 / 1")
    return runs["2"]


def test_stage_s_placements_rows_crossing_64_keys():
    """8 rows with prompts of 58-66 codes and 12 generated tokens (the generator of
    test_gpu_attn_chunk_scores.test_single_to_multi_transition_in_engine): rows go from the
    one-chunk aten-order path to flash chunks mid-call."""
    need_gpu()
    from t5gemma_tts_amd.engine import Utterance
    cfg, eng = _eager()
    rng = np.random.default_rng(5866)
    B = 8
    utts = []
    for i in range(B):
        tp = 58 + i + (i == 7)   # 58 .. 64, 66 codes
        x = rng.integers(3, 4000, size=int(rng.integers(4, 40))).tolist()
        utts.append(Utterance(x=x, y=rng.integers(0, 65536, size=tp).tolist() + [cfg.y_sep_token],
                              tgt_y_len=tp + 1 + 12))
    out = _stage_s_placements(eng, utts, list(range(700, 700 + B)), B)
    print("generated", [len(g) for g in out[0]["gen"]])
    # (rows 0-4 start at <= 63 keys: one of them generated its way past 64)
    assert max(len(out[0]["gen"][r]) for r in range(5)) >= 7


def test_stage_s_placements_sliding_window():
    """Layer 0 slides over a 100-key window (max_audio 448): rows with prompts of 299 and 130
    codes start their chunks at t - 99, a row of 70 is still inside the window."""
    need_gpu()
    from t5gemma_tts_amd.engine import Utterance
    cfg, eng = _eager(448, 100)
    assert cfg.backbone.sliding_window == 100
    rng = np.random.default_rng(100)
    utts = [Utterance(x=rng.integers(3, 4000, size=int(rng.integers(4, 40))).tolist(),
                      y=rng.integers(0, 65536, size=tp).tolist() + [cfg.y_sep_token], tgt_y_len=tp + 1 + 10)
            for tp in (299, 130, 70)]
    out = _stage_s_placements(eng, utts, [11, 12, 13], 3)
    assert sum(len(g) for g in out[0]["gen"]) > 3


@pytest.mark.parametrize("B", [3, 16])
def test_fp8_block_on_eager(B):
    """set_fp8_block(True) == off (the per-op FP8 launches) == the bf16 engine on W_q; the FP8
    whole-layer launch runs only with the switch on."""
    need_gpu()
    A, Bf = _fp8_pair()
    cfg = A.cfg
    L = cfg.backbone.num_decoder_layers
    utts = utterances(cfg, B, 510 + B, **ROWS)
    seeds = list(range(40, 40 + B))
    try:
        A.set_fp8_block(True)
        on = _run(A, utts, seeds)
        A.set_fp8_block(False)
        off = _run(A, utts, seeds)
    finally:
        A.set_fp8_block(False)
    ref = _run(Bf, utts, seeds)
    _same(on, off, B, "per-op P8")
    _same(on, ref, B, "bf16 on W_q")
    assert on[2] >= L and off[2] == 0, (on[2], off[2])
    assert len(on[0]["logits"]) > 1 and sum(len(g) for g in on[0]["gen"]) > B


def test_fp8_mlp_on_eager():
    """20 rows: set_fp8_mlp(True) == off == the bf16 engine on W_q; the FP8 MLP-half launch runs
    only with the switch on, the whole-layer launch not at all."""
    need_gpu()
    A, Bf = _fp8_pair()
    cfg = A.cfg
    L = cfg.backbone.num_decoder_layers
    B = 20
    utts = utterances(cfg, B, 530, **ROWS)
    seeds = list(range(70, 70 + B))
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
    assert on[3] >= L and off[3] == 0, (on[3], off[3])
    assert on[2] == 0 and off[2] == 0, (on[2], off[2])
    assert len(on[0]["logits"]) > 1 and sum(len(g) for g in on[0]["gen"]) > B

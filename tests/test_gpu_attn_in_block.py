"""The fast path's decode self attention as stage S of the persistent layer launch
(csrc/fused_attn.h fb_self_attn: the flash launch's arithmetic, one 64-key chunk per 4-wave
group spread over every workgroup, the holder of a (row, kv head)'s last chunk combining, att_self handed to the o-projection
in-launch) against the same step with the attention as its own flash launch
(attn.hip attn_decode_kernel<256, 2, true, true>): tokens and every logit row bitwise equal,
at the true 2b-2b widths (2 + 2 layers), for 1-16 rows with rows of one chunk (the aten-order
single-block path), of several chunks and of partial chunk triples; on a sliding-window layer
past its window; and a call whose rows need more tasks than workgroups keeps the separate
launch (same bits). Reference: [tf] modeling_t5gemma.py:264-304 (self attention in
PMDecoderLayer, hf_export/modeling_t5gemma_voice.py:256-323)."""
import numpy as np
import pytest

from tests.engine_cases import assert_same_run, both_loops, default_params, mid_engine, need_gpu, utterances

pytestmark = pytest.mark.gpu


def _run(eng, utts, p, seeds, on):
    eng.set_attn_in_block(on)   # 0 the separate flash launch, 1 stage S in front, 2 at the end
    before = eng.attn_in_block_launches()
    # host loop (every step's logits) and the graph-replayed on-device loop (tokens)
    out, fast = both_loops(eng, utts, seeds, p)
    return out, fast, eng.attn_in_block_launches() - before


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("B,tp_max", [(1, 1), (3, 300), (8, 400), (16, 300)])
def test_attention_in_block_bitwise_equal_to_flash_launch(B, tp_max, mode):
    need_gpu()
    cfg, eng = mid_engine(16, 448)
    utts = utterances(cfg, B, 60 + B, bare_first=True, tp_max=tp_max)   # row 0: one-chunk rows throughout
    p = default_params()
    seeds = list(range(900, 900 + B))
    on0, fon0, n_on0 = _run(eng, utts, p, seeds, mode)
    assert eng.attn_in_block_mode() == mode   # short rows: each mode takes its own placement
    off, foff, n_off = _run(eng, utts, p, seeds, 0)
    on1, fon1, n_on1 = _run(eng, utts, p, seeds, mode)
    assert n_off == 0 and n_on0 > 0 and n_on1 > 0   # stage S ran, and only when enabled
    assert_same_run(on0, off, B, "on/off")
    assert_same_run(on0, on1, B, "on/on")
    assert_same_run(fon0, foff, B, "graph on/off")
    assert_same_run(fon0, fon1, B, "graph on/on")
    assert sum(len(g) for g in on0["gen"]) > B


@pytest.mark.parametrize("mode", [1, 2])
def test_attention_in_block_sliding_window(mode):
    """Layer 0 slides over a 100-key window: rows past it start their chunks at t - 99."""
    need_gpu()
    cfg, eng = mid_engine(8, 448, window=100)
    utts = utterances(cfg, 6, 17, bare_first=True, tp_max=350)
    p = default_params()
    seeds = list(range(6))
    on, fon, n_on = _run(eng, utts, p, seeds, mode)
    off, foff, _ = _run(eng, utts, p, seeds, 0)
    assert n_on > 0
    assert_same_run(on, off, 6, "window")
    assert_same_run(fon, foff, 6, "window graph")


def test_attention_in_block_falls_back_past_two_passes():
    """16 rows of up to ~1 650 keys: 16 x 4 kv heads x 26 chunks = 1 664 chunk slots > two
    passes of 3 per workgroup (1 536), so the call keeps the separate flash launch -- the same
    bits either way."""
    need_gpu()
    cfg, eng = mid_engine(16, 1700)
    from t5gemma_tts_amd.engine import Utterance
    rng = np.random.default_rng(3)
    utts = [Utterance(x=rng.integers(3, 4000, size=20).tolist(),
                      y=rng.integers(0, 65536, size=1630).tolist() + [cfg.y_sep_token], tgt_y_len=1631 + 10)
            for _ in range(16)]
    p = default_params()
    seeds = list(range(16))
    on, fon, n_on = _run(eng, utts, p, seeds, 2)
    on1, fon1, n_on1 = _run(eng, utts, p, seeds, 1)
    off, foff, _ = _run(eng, utts, p, seeds, 0)
    assert n_on == 0 and n_on1 == 0
    assert_same_run(on, off, 16, "fallback")
    assert_same_run(on1, off, 16, "fallback 1")
    assert_same_run(fon, foff, 16, "fallback graph")


def test_tail_mode_falls_back_to_front_past_two_slots_per_worker():
    """16 rows of ~600 keys: 16 x 4 kv heads x 10 chunks = 640 > 2 slots per worker (480), so
    mode 2 runs stage S in front of each layer's o-projection (<= 3 per workgroup) -- still no
    separate attention launch, the same bits."""
    need_gpu()
    from t5gemma_tts_amd.engine import Utterance
    cfg, eng = mid_engine(16, 640)
    rng = np.random.default_rng(4)
    utts = [Utterance(x=rng.integers(3, 4000, size=20).tolist(),
                      y=rng.integers(0, 65536, size=590).tolist() + [cfg.y_sep_token], tgt_y_len=591 + 10)
            for _ in range(16)]
    p = default_params()
    seeds = list(range(16))
    on, fon, n_on = _run(eng, utts, p, seeds, 2)
    assert eng.attn_in_block_mode() == 1   # the placement the decode launches took: in front
    off, foff, _ = _run(eng, utts, p, seeds, 0)
    assert eng.attn_in_block_mode() == 0
    assert n_on > 0
    assert_same_run(on, off, 16, "front fallback")
    assert_same_run(fon, foff, 16, "front fallback graph")


@pytest.mark.parametrize("tp,max_audio", [(1240, 1300), (2480, 2560)])
def test_attention_in_block_long_rows(tp, max_audio):
    """Rows past 1 024 keys in the launch (round 6): 8 rows of ~1 250 keys (20 chunks: the
    combine reads its records in two batches of 16, as the flash launch does; one pass of 3
    slots per workgroup, front mode) and of ~2 500 keys (40 chunks: two passes of 3 nb slots).
    Bitwise equal to the separate flash launch, stage S in every decode launch. Reference: the
    reference serves 100 s prompts (inference_commandline_hf.py:91, 181)."""
    need_gpu()
    from t5gemma_tts_amd.engine import Utterance
    cfg, eng = mid_engine(8, max_audio)
    rng = np.random.default_rng(tp)
    utts = [Utterance(x=rng.integers(3, 4000, size=20).tolist(),
                      y=rng.integers(0, 65536, size=tp - 8 * i).tolist() + [cfg.y_sep_token],
                      tgt_y_len=tp - 8 * i + 1 + 12)
            for i in range(8)]
    p = default_params()
    seeds = list(range(8))
    on, fon, n_on = _run(eng, utts, p, seeds, 2)
    assert eng.attn_in_block_mode() == 1   # past the tail's 2 slots per worker: front mode
    off, foff, n_off = _run(eng, utts, p, seeds, 0)
    assert n_off == 0 and n_on >= 2 * 12   # stage S ran in the decode launches
    assert_same_run(on, off, 8, "long")
    assert_same_run(fon, foff, 8, "long graph")

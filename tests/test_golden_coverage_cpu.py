"""What the prompt-length goldens of the codec encoder and the Whisper decoder exist for, read
from the fixtures alone (no GPU): a regeneration at a shorter length, another stride or another
split of the teacher-forced sequence fails here instead of silently dropping what
tests/test_gpu_codec_enc.py and tests/test_gpu_whisper.py cover with them."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

AQ, AK = 128, 64            # attn_relkey_kernel / whs_attn_kernel: queries per block, keys per tile
SPLIT = 256                 # whs_attn_dec_kernel: keys per split
MAX_BYTES = 200 * 1000


def _enc(name):
    with open(os.path.join(GOLDEN, f"golden_codec_enc_{name}.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLDEN, f"golden_codec_enc_{name}.npz"))


def _snake_lengths(meta):
    """The lengths the anti-aliased activations run at: each block's input, then the frames."""
    T = meta["n_codes"]
    L = T * int(np.prod(meta["config"]["strides"]))
    out = []
    for s in meta["config"]["strides"]:
        out.append(L)
        L //= s
    assert L == T
    return out + [T]


@pytest.mark.parametrize("name,frames", [("tiny_long", 334), ("tiny_t200", 200), ("tiny_short", 3),
                                         ("full16k_mid", 134)])
def test_encoder_long_goldens_are_consistent(name, frames):
    meta, z = _enc(name)
    T = meta["n_codes"]
    assert T == frames == meta["n_samples"] // 320 + 1
    assert "wav" not in z.files                      # results only: the test rebuilds the waveform
    stride = meta["feature_row_stride"]
    assert z["features"].shape == (-(-T // stride), 160)
    assert z["codes"].shape == (T,) and z["latent"].shape == (T, len(meta["config"]["levels"]))
    assert meta["frames_near_boundary"] <= 0.10 * T
    assert os.path.getsize(os.path.join(GOLDEN, f"golden_codec_enc_{name}.npz")) < MAX_BYTES


def test_encoder_long_goldens_reach_the_tiles_and_the_left_clamp():
    long_, _ = _enc("tiny_long")
    mid, _ = _enc("full16k_mid")
    for meta, blocks, tiles in ((long_, 3, 6), (mid, 2, 3)):
        T = meta["n_codes"]
        assert T > AQ and T > meta["config"]["rel_left"] + 1      # a second query block, a clamped distance
        assert -(-T // AQ) >= blocks and -(-T // AK) >= tiles
        assert T % AK and T % AQ                                   # ragged last tile and block
        assert T - (meta["config"]["dw_kernel"] - 1) > 100         # the conv module's steady state
    assert mid["config"]["sem_hidden"] == 1024 and mid["config"]["sem_heads"] == 16
    short, _ = _enc("tiny_short")
    assert short["n_codes"] < short["config"]["dw_kernel"]         # all causal edge


def test_one_encoder_golden_runs_the_4_wide_snake_at_every_stage():
    meta, _ = _enc("tiny_t200")
    lens = _snake_lengths(meta)
    assert len(lens) == 6 and all(L % 4 == 0 and L >= 8 for L in lens), lens
    # the goldens before it never did at the last two
    for old in ("tiny", "full16k", "tiny_long"):
        assert any(L % 4 for L in _snake_lengths(_enc(old)[0])[-2:])


@pytest.mark.parametrize("name", ["tiny", "turbo"])
def test_whisper_long_golden_fills_the_text_context(name):
    with open(os.path.join(GOLDEN, f"golden_whisper_{name}_long.json")) as f:
        meta = json.load(f)
    path = os.path.join(GOLDEN, f"golden_whisper_{name}_long.npz")
    z = np.load(path)
    d = meta["model_dims"]
    n = len(meta["teacher_tokens"])
    assert n == d["n_text_ctx"] == 448
    assert meta["prefill"] > AQ and meta["prefill"] > 4        # two query blocks; the tiled GEMM, not the GEMV
    assert meta["prefill"] < SPLIT < n and n % SPLIT           # single steps cross a split; ragged last split
    assert z["logits_sub"].shape == (n, len(z["sub"])) and z["argmax"].shape == z["margin"].shape == (n,)
    assert np.array_equal(z["sub"], np.arange(0, d["n_vocab"], meta["col_stride"]))
    assert 0 <= z["argmax"].min() and z["argmax"].max() < d["n_vocab"] and (z["margin"] >= 0).all()
    assert meta["rows_within_twice_bound"] <= 0.05 * n
    assert os.path.getsize(path) < MAX_BYTES
    # the short golden's model and window: one recognizer serves both
    with open(os.path.join(GOLDEN, f"golden_whisper_{name}.json")) as f:
        short = json.load(f)
    for k in ("weight_seed", "audio_seed", "audio_seconds", "tok_seed", "content_frames", "model_dims"):
        assert meta[k] == short[k], k

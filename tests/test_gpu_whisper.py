"""Whisper recognizer on the GPU (whs_* C ABI) against transformers'
WhisperForConditionalGeneration goldens (tests/golden/make_golden_whisper.py) at test
dims and at large-v3-turbo dims (128 mels, 32 x 1280 encoder, 4 x 1280 decoder):

* log-mel vs the oracle's torch.stft restatement of openai's log_mel_spectrogram
  (fp32 DFT GEMM vs FFT: <= 2e-3 on the (x + 4) / 4 scale);
* encoder output of the first window and teacher-forced decoder logits (prefill, then one
  token at a time through the self-attention cache) within 2e-3 x their RMS, argmax equal;
* detect_language's choice, and the tokens of transcribe(audio, temperature=0) -- the
  host control flow over the GPU logits -- equal to the oracle's.
* a second teacher-forced sequence that fills the 448-token text context (golden_whisper_*_long:
  a condition_on_previous_text prompt of 203 tokens, then the longest decode), fed as one
  prefill plus single steps and again in chunks of 2, 4, 5 and 130: the tiled GEMM in the
  decoder, causal attention over two query blocks and at an offset, and a self cache whose
  splits cross 256 keys up to the last row.
One recognizer per config serves every test of this file (each test sets the state it needs).
Parity against the openai-whisper package itself is unpinned (absent)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, GOLDEN)


def _load(name):
    with open(os.path.join(GOLDEN, f"golden_whisper_{name}.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN, f"golden_whisper_{name}.npz")))


_MODELS = {}


def _setup(name, tmp_path):
    if name not in _MODELS:
        _MODELS[name] = _build(name, tmp_path)
    return _MODELS[name]


def _build(name, tmp_path):
    from t5gemma_tts_amd import whisper_asr as w
    from make_golden_codec_enc import test_wave
    from whisper_oracle import write_synthetic_tiktoken
    meta, z = _load(name)
    dims = w.WhisperDims(**meta["model_dims"])
    p = str(tmp_path / "v.tiktoken")
    write_synthetic_tiktoken(p, 50257, meta["tok_seed"])
    tok = w.WhisperTokenizer.from_tiktoken(p, dims.num_languages)
    m = w.WhisperModel(dims, w.synthetic_weights(dims, meta["weight_seed"]), device="cuda:0", max_seconds=30.0,
                       tokenizer=tok)
    audio = test_wave(int(meta["audio_seconds"] * 16000), meta["audio_seed"])
    return w, meta, z, m, tok, audio


@pytest.mark.parametrize("name", ["tiny", "turbo"])
def test_whisper_model_vs_transformers_golden(name, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from whisper_oracle import ref_log_mel
    w, meta, z, m, tok, audio = _setup(name, tmp_path)
    mel = m.log_mel(audio, out=True).cpu()
    ref = ref_log_mel(audio, m.dims.n_mels).T
    merr = (mel - ref).abs().max().item()
    assert m.mel_frames == meta["content_frames"] + 3000
    feat = m.encode(0, meta["content_frames"], out=True).cpu()[::25]
    ref_feat = torch.from_numpy(z["feat_rows"])
    ferr = ((feat - ref_feat).abs().max() / ref_feat.pow(2).mean().sqrt()).item()
    toks = meta["teacher_tokens"]
    rows = [m.logits(toks[:3], 0).cpu().clone()]
    for i in range(3, len(toks)):
        rows.append(m.logits(toks[i:i + 1], i).cpu().clone())
    lg = torch.cat(rows, 0)
    sub = torch.from_numpy(z["sub"]).long()
    ref_lg = torch.from_numpy(z["logits_sub"])
    lerr = ((lg[:, sub] - ref_lg).abs().max() / ref_lg.pow(2).mean().sqrt()).item()
    print(f"{name}: mel max err {merr:.2e}, encoder err/rms {ferr:.2e}, logits err/rms {lerr:.2e}")
    assert merr <= 2e-3, merr
    assert ferr <= 2e-3, ferr
    assert lerr <= 2e-3, lerr
    assert lg.argmax(-1).tolist() == meta["logit_argmax"]


LONG_PASSES = {"prefill_then_steps": [203], "chunks_2_4_5_130_then_steps": [2, 4, 5, 130]}


@pytest.mark.parametrize("chunks", list(LONG_PASSES))
@pytest.mark.parametrize("name", ["tiny", "turbo"])
def test_whisper_full_context_teacher_forcing(name, chunks, tmp_path):
    """448 teacher-forced tokens against golden_whisper_<name>_long, at the bound of the short
    sequence (2e-3 x the logits' RMS). prefill_then_steps: 203 tokens at once (the tiled GEMM,
    causal attention over two query blocks), then 245 single steps to position 447 (self-cache
    splits crossing 256 keys with a ragged second split). chunks_...: the same tokens as 2 + 4
    (the GEMV at M = 2 and 4), 5 + 130 (the tiled GEMM and the causal kernel at q_off > 0), then
    single steps. The argmax is equal on every row whose golden top-2 margin exceeds twice the
    bound; the other rows are at most 5 % (4 of 448 in the tiny golden, none in turbo).
    MI355X: logits within 3.0e-6 / 3.0e-6 x RMS (tiny, the two passes) and 3.8e-6 / 3.9e-6 (turbo),
    the argmax equal on all 448 rows in all four."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    w, meta, z, m, tok, audio = _setup(name, tmp_path)
    with open(os.path.join(GOLDEN, f"golden_whisper_{name}_long.json")) as f:
        lmeta = json.load(f)
    lz = np.load(os.path.join(GOLDEN, f"golden_whisper_{name}_long.npz"))
    assert lmeta["weight_seed"] == meta["weight_seed"] and lmeta["audio_seed"] == meta["audio_seed"]
    toks = lmeta["teacher_tokens"]
    assert len(toks) == m.dims.n_text_ctx and LONG_PASSES["prefill_then_steps"] == [lmeta["prefill"]]
    m.log_mel(audio)
    m.encode(0, lmeta["content_frames"])
    sub = torch.from_numpy(lz["sub"]).long().cuda()
    rows, arg, pos = [], [], 0
    sizes = LONG_PASSES[chunks]
    for n in sizes + [1] * (len(toks) - sum(sizes)):
        lg = m.logits(toks[pos:pos + n], pos)
        rows.append(lg[:, sub].clone())
        arg.append(lg.argmax(-1))
        pos += n
    assert pos == len(toks)
    got, arg = torch.cat(rows, 0).cpu(), torch.cat(arg, 0).cpu()
    ref = torch.from_numpy(lz["logits_sub"])
    rms = ref.pow(2).mean().sqrt().item()
    lerr = (got - ref).abs().max().item() / rms
    excused = torch.from_numpy(lz["margin"]) <= 2 * 2e-3 * rms
    same = arg == torch.from_numpy(lz["argmax"]).long()
    print(f"{name} {chunks}: logits err/rms {lerr:.2e}, argmax equal {int(same.sum())}/{same.numel()}, "
          f"{int(excused.sum())} rows within twice the bound")
    assert lerr <= 2e-3, lerr
    assert bool((same | excused).all()), torch.nonzero(~(same | excused)).view(-1).tolist()
    assert int(excused.sum()) == lmeta["rows_within_twice_bound"] and excused.sum() <= 0.05 * excused.numel()


@pytest.mark.parametrize("name", ["tiny", "turbo"])
def test_whisper_transcribe_vs_oracle(name, tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    w, meta, z, m, tok, audio = _setup(name, tmp_path)
    m.log_mel(audio)
    lang, probs = m.detect_language(tok.with_language("en"))
    assert lang == meta["language"]
    for code, p in meta["language_top5"]:
        assert abs(probs[code] - p) < 1e-3 * max(p, 1e-3) + 1e-5, (code, probs[code], p)
    r = m.transcribe(audio, temperature=0.0)
    got = [s["tokens"] for s in r["segments"]]
    want = [s["tokens"] for s in meta["segments"]]
    print(f"{name}: language {r['language']}, {len(got)} segments, tokens equal: {got == want}")
    assert r["language"] == meta["transcribe_language"]
    assert got == want
    for s, g in zip(r["segments"], meta["segments"]):
        assert abs(s["start"] - g["start"]) < 1e-9 and abs(s["end"] - g["end"]) < 1e-9


def test_transcribe_wav_file_and_capacity(tmp_path):
    """A reference WAV at 44.1 kHz is resampled to 16 kHz as openai's ffmpeg loader does;
    audio longer than the recognizer's capacity is refused."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from t5gemma_tts_amd.audio import resample, write_wav
    w, meta, z, m, tok, audio = _setup("tiny", tmp_path)
    path = str(tmp_path / "ref.wav")
    write_wav(path, resample(audio[None], 16000, 44100)[0], 44100)
    r = m.transcribe(path, temperature=0.0, language="en")
    assert r["language"] == "en" and isinstance(r["text"], str)
    with pytest.raises(ValueError):
        m.log_mel(torch.zeros(31 * 16000))

"""The inputs tests/engine_cases.py and tests/kernel_cases.py generate are the ones the GPU tests
were written on: SHA-256 of what the per-file helpers drew before they were merged (recorded
from those helpers, never from the shared ones), for every distinct call shape. A helper that
drew something else would leave a GPU test passing on cases it was not written for. CPU only.

Each hash was recorded at the commit before the merge, with _utt_hash / _bits_hash below applied to
the call named next to it (cfg as _cfg() makes it); the three copies of the default generator and
the two of _hdr and of _run's draw gave equal hashes there."""
import dataclasses
import hashlib
import json
import os

import numpy as np
import torch

from conftest import GOLDEN
from tests import engine_cases as ec
from tests import kernel_cases as kc


def _utt_hash(utts):
    h = hashlib.sha256()
    for u in utts:
        for part in (u.x, u.y, [u.tgt_y_len]):
            a = np.asarray(part, dtype=np.int64)
            h.update(np.int64(a.size).tobytes() + a.tobytes())
    return h.hexdigest()


def _bits_hash(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()


def _cfg():
    from t5gemma_tts_amd.config import named_config
    meta = json.load(open(os.path.join(GOLDEN, "golden_mid.json")))
    return named_config(meta["config"], **meta["config_kw"])   # no weights: utterances reads y_sep_token only


def test_utterances_default_is_the_fused_generator():
    """test_gpu_fused / test_gpu_fp8_engine / test_gpu_time_hooks."""
    cfg = _cfg()
    # test_gpu_fused._utts(cfg, 8, 48) and (cfg, 32, 72)
    assert _utt_hash(ec.utterances(cfg, 8, 48)) == "9bd6c9a2f8779b22fc396c1a34f3435f4ff052fd6b0cc27a0a335892344e1c3a"
    assert _utt_hash(ec.utterances(cfg, 32, 72)) == "c3d17ac8b28640d68f724db11e1e93c0a8c39d0159730cda9410934b22b6a6a2"


def test_utterances_max_text_is_the_xlayer_generator():
    # test_gpu_xlayer._utts(cfg, 8, 98, max_text=64)
    assert _utt_hash(ec.utterances(_cfg(), 8, 98, max_text=64)) == \
        "84039a6b14a81943c0774722b759f1bbe947c40deb5976e6d54c4f891dbcda23"


def test_utterances_bare_first_is_the_attn_in_block_generator():
    # test_gpu_attn_in_block._utts(cfg, 8, 68, 400)
    assert _utt_hash(ec.utterances(_cfg(), 8, 68, bare_first=True, tp_max=400)) == \
        "40edfc717cda3caa5b06fce6214844840d535d357f7abcd96af1026ed7e01b0b"


def test_utterances_text_lens_is_the_rows32_generator():
    # test_gpu_fused_rows32._utts(cfg, 17, 157)
    utts = ec.utterances(_cfg(), 17, 157, bare_first=True, text_lens={1: 64, 2: 4})
    assert _utt_hash(utts) == "57272d63af36a126e68d9ff71a815227ff30d72a56adda5091e41c9e89c7574f"
    assert (len(utts[0].y), len(utts[1].x), len(utts[2].x)) == (0, 64, 4)


def test_hdr_bf16_draw():
    # test_gpu_exact._hdr((4, 2304), torch.Generator().manual_seed(3))
    got = kc.hdr_bf16((4, 2304), torch.Generator().manual_seed(3))
    assert _bits_hash(got) == "aa06e4773d78173a2bb3124a7a08e6e964beb00fefec45c83d9b606eb8eeda59"


def test_decode_attention_call_draw():
    """decode_attention_call(L, B=4, ..., cap=65, seed=65) draws attn_inputs(65, 4, 8, 4, 256, 4, 65)."""
    # q, K, V as prepare() saw them in test_gpu_attention._run(65, 4, [65, 64, 3, 1], cap=65, seed=65, prepare=...)
    q, K, V = kc.attn_inputs(65, 4, 8, 4, 256, 4, 65)
    assert (q.shape, K.shape, V.shape) == ((4, 8, 256), (4, 4, 65, 256), (4, 4, 65, 256))
    assert _bits_hash(q, K, V) == "7c5e62dedce689d9c82685f9513fe371272ec60d4010894a396756053e200e48"


def test_mid_config_is_made_once(monkeypatch):
    """The second call returns the first call's state dict; a window changes the config only.
    (The weights themselves are stubbed: 657 M parameters take seconds to draw.)"""
    from t5gemma_tts_amd import weights
    calls = []

    def fake(cfg, seed):
        calls.append(seed)
        return {"seed": seed}

    monkeypatch.setattr(weights, "synthetic_weights", fake)
    ec._mid_config.cache_clear()
    try:
        cfg, sd = ec.mid_config()
        cfg2, sd2 = ec.mid_config(None)
        wcfg, wsd = ec.mid_config(window=100)
        assert sd2 is sd and cfg2 is cfg and wsd is sd and len(calls) == 1
        assert wcfg.backbone.sliding_window == 100 != cfg.backbone.sliding_window
        assert calls[0] == json.load(open(os.path.join(GOLDEN, "golden_mid.json")))["weight_seed"]
        # attn_implementation likewise: the config only, alone and together with a window
        ecfg, esd = ec.mid_config(attn_implementation="eager")
        bcfg, bsd = ec.mid_config(window=100, attn_implementation="eager")
        assert esd is sd and bsd is sd and len(calls) == 1
        assert cfg.backbone.attn_implementation == "sdpa" and cfg.backbone.softcap == 0.0
        assert ecfg.backbone.attn_implementation == "eager" and ecfg.backbone.softcap == 50.0
        assert ecfg.backbone.sliding_window == cfg.backbone.sliding_window
        assert bcfg.backbone.softcap == 50.0 and bcfg.backbone.sliding_window == 100
        assert ecfg == dataclasses.replace(cfg, backbone=dataclasses.replace(cfg.backbone, attn_implementation="eager"))
    finally:
        ec._mid_config.cache_clear()   # drop the stub's result


def test_mid_weights_do_not_depend_on_attn_implementation():
    """mid_config hands the eager engine the state dict it drew for the config's own sdpa: the
    weights drawn for the eager config are the same (the digest golden_mid.json records)."""
    from t5gemma_tts_amd.weights import state_dict_digest, synthetic_weights
    meta = json.load(open(os.path.join(GOLDEN, "golden_mid.json")))
    cfg = _cfg()
    ecfg = dataclasses.replace(cfg, backbone=dataclasses.replace(cfg.backbone, attn_implementation="eager"))
    assert cfg.backbone.softcap == 0.0 and ecfg.backbone.softcap == 50.0
    assert state_dict_digest(synthetic_weights(ecfg, meta["weight_seed"])) == meta["weight_sha256"]


def test_header_symbols_are_the_bound_signatures():
    from t5gemma_tts_amd import _lib
    syms = ec.header_symbols("t5gtts.h", "t5g")
    assert len(syms) >= 20 and set(syms) == set(_lib.SIGNATURES), set(syms) ^ set(_lib.SIGNATURES)

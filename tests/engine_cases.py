"""Set-up shared by the engine-level tests: the one GPU skip, the ctypes pointer helpers, the
golden_mid engine (true 2b-2b widths, 2 + 2 layers) and its ragged utterances, the host-loop /
graph-loop pair of generate() calls with its bitwise comparison, the golden loaders, the
teacher-forced replay through the CPU oracle, and the header scan of the CPU ABI tests.
tests/test_engine_cases_cpu.py pins, with no GPU, the inputs these helpers generate to the ones
the tests were written on. Kernel-level inputs and references are in tests/kernel_cases.py.
"""
import ctypes as C
import dataclasses
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, gpu_available


def need_gpu():
    if not gpu_available():
        pytest.skip("needs the MI355X")


def stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------
# goldens
def load_golden(name):
    """(meta, arrays) of tests/golden/<name>.json and, where there is one, <name>.npz."""
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        meta = json.load(f)
    npz = os.path.join(GOLDEN, name + ".npz")
    return meta, (dict(np.load(npz)) if os.path.exists(npz) else {})


def golden_params(c, oracle=False):
    """A golden case's sampling parameters, for the engine or (oracle=True) for the CPU oracle."""
    if oracle:
        from oracle.t5g_oracle import SamplerParams as P
    else:
        from t5gemma_tts_amd.engine import SamplingParams as P
    return P(top_k=c["top_k"], top_p=c["top_p"], min_p=c["min_p"], temperature=c["temperature"],
             stop_repetition=c["stop_repetition"], silence_tokens=tuple(c["silence_tokens"]))


def topk_agree(g, r, k, tol):
    """Top-k index sets of g and r equal, except members whose value is within ``tol`` of
    the k-th value (ties at the cut may legitimately swap)."""
    gv, gi = torch.topk(g.float(), k)
    rv, ri = torch.topk(r.float(), k)
    cut = min(gv[-1].item(), rv[-1].item())
    sg = {int(i) for i, v in zip(gi, gv) if v.item() > cut + tol}
    sr = {int(i) for i, v in zip(ri, rv) if v.item() > cut + tol}
    return sg <= set(ri.tolist()) and sr <= set(gi.tolist())


def teacher_forced_check(cfg, sd, utt, params_o, seed, gpu_out, rtol):
    """Replay the GPU's token sequence through the CPU oracle. At every step:
    (a) the reference sampler fed the GPU's logits + the same noise returns the GPU's
        token (sampler exactness, incl. tie order and stop rules);
    (b) the GPU logits match the oracle logits under the identical history
        (bf16 GEMM accumulation order => within a few bf16 ulps, rtol of max |logit|).
    Returns (max relative logit error, number of exactly equal logit rows)."""
    import copy
    from oracle.t5g_oracle import T5GemmaTTSOracle, draw_noise, sample_helper
    orc = T5GemmaTTSOracle(cfg, sd)
    ctx = orc.prepare(utt.x, utt.y, utt.tgt_y_len)
    st = ctx["state"]
    gen = torch.Generator().manual_seed(int(seed))
    toks = gpu_out["gen"][0].tolist()
    worst, exact_rows = 0.0, 0
    for t, tok in enumerate(toks):
        lo = orc.step_logits(ctx)
        lg = gpu_out["logits"][t][0].cpu()
        noise = draw_noise(gen, lo.shape[-1])
        scale = lo.float().abs().max().item()
        err = (lg.float() - lo.float()).abs().max().item() / max(scale, 1e-6)
        worst = max(worst, err)
        exact_rows += int(torch.equal(lg, lo))
        st_g = copy.deepcopy(st)
        tok_g, _ = sample_helper(lg.clone(), params_o, st_g, noise, eos=cfg.eog_inference,
                                 encodec_sr=cfg.encodec_sr, extra_cutoff=cfg.extra_cutoff,
                                 text_guard_frames_per_token=cfg.text_guard_frames_per_token)
        assert tok_g == tok, f"step {t}: reference sampler on GPU logits -> {tok_g}, GPU sampled {tok}"
        ctx["state"] = st = st_g
        st.cur_num_gen += 1
        st.current_length += 1
        if tok == cfg.eog_inference:
            assert t == len(toks) - 1
            break
        orc.advance(ctx, tok)
    assert worst <= rtol, worst
    return worst, exact_rows


def bf16_bits(t):
    return t.contiguous().view(torch.int16).numpy()


def header_symbols(header_file, prefix):
    """The functions include/<header_file> declares as prefix_name(, comments stripped."""
    src = open(os.path.join(REPO, "include", header_file)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % prefix, src)))


# ---------------------------------------------------------------------------
# the golden_mid engine
@functools.lru_cache(maxsize=None)
def _mid_config():
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.weights import synthetic_weights
    meta, _ = load_golden("golden_mid")
    cfg = named_config(meta["config"], **meta["config_kw"])
    return cfg, synthetic_weights(cfg, meta["weight_seed"])


def mid_config(window=None, attn_implementation=None):
    """(cfg, sd) of golden_mid, made once per process (sd is 657 M synthetic parameters that the
    engine only reads); window: the sliding layers' window instead of the config's;
    attn_implementation: "eager" (the 50.0 tanh logit softcap on) or "sdpa" instead of the
    config's (the weights depend on neither)."""
    cfg, sd = _mid_config()
    kw = {}
    if window is not None:
        kw["sliding_window"] = window
    if attn_implementation is not None:
        kw["attn_implementation"] = attn_implementation
    if kw:
        cfg = dataclasses.replace(cfg, backbone=dataclasses.replace(cfg.backbone, **kw))
    return cfg, sd


def mid_engine(max_batch, max_audio=128, window=None, attn_implementation=None, **engine_kw):
    """(cfg, a fresh engine) on golden_mid with max_text 64 and max_gen 40."""
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    cfg, sd = mid_config(window, attn_implementation)
    return cfg, T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=max_batch, max_text=64, max_audio=max_audio,
                                 max_gen=40, **engine_kw)


def utterances(cfg, n, seed, *, max_text=40, tp_max=40, bare_first=False, text_lens=None):
    """n ragged rows: 4 .. max_text - 1 text ids (text_lens: {row: length}, set without a draw),
    a prompt of 0 .. tp_max - 1 codes (bare_first: row 0 has none, without a draw) and 8 .. 29
    tokens to generate."""
    from t5gemma_tts_amd.engine import Utterance
    rng = np.random.default_rng(seed)
    utts = []
    for i in range(n):
        nx = text_lens[i] if text_lens and i in text_lens else int(rng.integers(4, max_text))
        x = rng.integers(3, 4000, size=nx).tolist()
        tp = 0 if bare_first and i == 0 else int(rng.integers(0, tp_max))
        y = rng.integers(0, 65536, size=tp).tolist() + ([cfg.y_sep_token] if tp else [])
        utts.append(Utterance(x=x, y=y, tgt_y_len=len(y) + int(rng.integers(8, 30))))
    return utts


def default_params():
    from t5gemma_tts_amd.engine import SamplingParams
    return SamplingParams(top_k=30, top_p=0.9, temperature=0.8)


def both_loops(eng, utts, seeds, params=None, host_first=True):
    """(host, fast): the fast kernels step by step from the host loop (tokens and every step's
    logits) and the graph-replayed on-device loop (tokens), run in that order or the other (the
    engine's graphs and counters make the order observable)."""
    p = default_params() if params is None else params

    def host():
        return eng.generate(utts, p, seeds=seeds, parity=True, exact=False, record_logits=True)

    def fast():
        return eng.generate(utts, p, seeds=seeds)

    if host_first:
        h = host()
        return h, fast()
    f = fast()
    return host(), f


def assert_same_run(a, b, B, tag):
    """Two generate() results bitwise: the tokens of rows 0 .. B - 1 and, where logits were
    recorded, every step's logits."""
    for r in range(B):
        assert a["gen"][r].tolist() == b["gen"][r].tolist(), (tag, r)
    if "logits" not in a:   # the graph-replayed loop: tokens only
        return
    assert len(a["logits"]) == len(b["logits"]), tag
    for s, (la, lb) in enumerate(zip(a["logits"], b["logits"])):
        assert torch.equal(la.view(torch.int16), lb.view(torch.int16)), (tag, s)

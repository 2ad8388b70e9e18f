"""The device sampler's per-row state machine (csrc/sampler.hip: sampler_fast_kernel,
sampler_kernel, finish_row) on the rule cases of tests/sampler_cases.py, against the oracle's
sample_helper extended with the capacity rules, the counters and next_pos
(sampler_cases.expected; the same expectation pins t5g_host_sample in
tests/test_sampler_rules_cpu.py).

Engines as in tests/test_gpu_sampler.py: tiny backbone, vocabulary 65536 + 5, max_gen 128; a
second config has text_guard_frames_per_token = 10 and extra_cutoff = 0.25. Noise is a
[B][1][V] buffer with noise_steps = 1, so every row reads its own slot whatever its
cur_num_gen. Each launch mixes rows the fast path finishes, rows it hands to the single-block
kernel, done rows and stalled rows.
"""
import ctypes as C
import functools

import pytest
import torch

from tests import sampler_cases as SC
from tests.engine_cases import stream

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V_BIG, EOS_BIG = 65541, 65539
V_TINY, EOS_TINY = 69, 67
ROWS = 8
PAD_LOGIT = 30000.0     # beyond column V of the logits rows: a kernel reading past V would pick it
ALL = SC.all_cases()


@functools.lru_cache(maxsize=None)
def _engine(cfg_key, single_block, tiny_vocab):
    import t5gemma_tts_amd  # noqa: F401
    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import T5GemmaTTSEngine
    from t5gemma_tts_amd.weights import synthetic_weights
    cfg = named_config("tiny")
    if not tiny_vocab:
        cfg.audio_vocab_size = 65536
        cfg.empty_token, cfg.eog, cfg.audio_pad_token, cfg.eos, cfg.y_sep_token = 65536, 65537, 65538, 65539, 65540
    cfg.text_guard_frames_per_token = SC.CFGS[cfg_key]["text_guard"]
    cfg.extra_cutoff = SC.CFGS[cfg_key]["extra_cutoff"]
    eng = T5GemmaTTSEngine(cfg, synthetic_weights(cfg, 3), device="cuda:0", max_batch=ROWS, max_text=16,
                           max_audio=SC.MAX_AUDIO, max_gen=SC.MAX_GEN)
    c = eng._cfg
    assert (c.eos, c.eos_guard, c.text_guard, c.progress_scale, c.n_audio_tokens) == \
        (EOS_TINY if tiny_vocab else EOS_BIG, SC.EOS_GUARD, SC.CFGS[cfg_key]["text_guard"], SC.PROGRESS_SCALE,
         V_TINY if tiny_vocab else V_BIG)
    assert c.budget_extra == int(SC.ENCODEC_SR) * SC.CFGS[cfg_key]["extra_cutoff"]
    _lib.check(eng.L.t5g_engine_set_audio_max(eng.h, SC.KEY_BOUND), "set_audio_max")
    if single_block:
        _lib.check(eng.L.t5g_engine_set_sampler_path(eng.h, 1), "set_sampler_path")
    return eng


def _launches(cases):
    """The cases eight rows at a time. Rows of one launch share an engine config and a logits
    leading dimension; within such a bucket the four kinds of row are dealt in rotation, so
    the launches that hold done / stalled rows hold fast and fallback rows as well."""
    buckets = {}
    for c in cases:
        buckets.setdefault((c["cfg"], c["ld_pad"]), []).append(c)
    out = []
    for key in sorted(buckets):
        queues = {k: [c for c in buckets[key] if SC.row_kind(c) == k] for k in ("fast", "fallback", "done", "stalled")}
        dealt = []
        while any(queues.values()):
            for k in ("fast", "done", "fallback", "stalled", "fast", "fast"):
                if queues[k]:
                    dealt.append(queues[k].pop(0))
        out += [dealt[i:i + ROWS] for i in range(0, len(dealt), ROWS)]
    return out


def _upload_logits(rows_bf16, V, ld):
    d = torch.full((len(rows_bf16), ld), PAD_LOGIT, dtype=BF16)
    for b, r in enumerate(rows_bf16):
        d[b, :V] = r
    return d.cuda()


def _setup(eng, cases, V, noise_dev, noise_steps):
    from t5gemma_tts_amd import _lib
    rows, sts = SC.lib_rows_states(cases, V)
    tk, ntk, sl, nsl = SC.shared_lists()
    _lib.check(eng.L.t5g_sampler_setup(eng.h, len(cases), rows, sts, tk, ntk, sl, nsl,
                                       C.c_void_p(noise_dev.data_ptr()) if noise_dev is not None else None,
                                       noise_steps, stream()), "setup")
    return sts


def _sample(eng, B, dlg):
    from t5gemma_tts_amd import _lib
    _lib.check(eng.L.t5g_sample_only(eng.h, B, C.c_void_p(dlg.data_ptr()), dlg.shape[1], stream()), "sample")
    out = (_lib.SamplerState * B)()
    flags = (C.c_int32 * B)()
    _lib.check(eng.L.t5g_read_step(eng.h, out, flags, B, stream()), "read_step")
    toks = (C.c_int32 * (B * SC.MAX_GEN))()
    _lib.check(eng.L.t5g_read_tokens(eng.h, toks, B, stream()), "read_tokens")
    return out, list(flags), [list(toks[b * SC.MAX_GEN:(b + 1) * SC.MAX_GEN]) for b in range(B)]


def _one_step(eng, cases, V, eos, reference_noise=True):
    exps = [SC.expected(c, V, eos) for c in cases]
    noise = torch.stack([e["noise"] for e in exps])[:, None].contiguous().cuda() if reference_noise else None
    init = _setup(eng, cases, V, noise, 1 if reference_noise else 0)
    dlg = _upload_logits([e["logits"] for e in exps], V, V + cases[0]["ld_pad"])
    out, flags, toks = _sample(eng, len(cases), dlg)
    return exps, init, out, flags, toks


def _init_dict(st):
    return {f: getattr(st, f) for f in SC.STATE_FIELDS}


def _check_row(case, exp, init, out, flag, toks, single_block):
    """Asserts one row of a reference-noise launch; returns True when the row is skipped (a
    stalled tie cut on the single-block kernel) and False when it was compared in full."""
    name, empty = case["name"], [-1] * SC.MAX_GEN
    start = _init_dict(init)
    if start["done"]:
        assert SC.state_mismatches(out, start) == [], name     # no state change
        assert toks == empty, name                              # no token written
        return False
    if flag & 4:
        # the only excuse: a tie order the single-block kernel leaves to the host's std::sort
        assert exp["tie"], name
        assert single_block, name
        assert SC.state_mismatches(out, dict(start, done=2)) == [], name
        assert toks == empty, name
        return True
    want = dict(exp["state"], ambiguous_steps=start["ambiguous_steps"] + (flag & 1))
    assert out.last_token == exp["token"], (name, out.last_token, exp["token"], exp["sampled"])
    assert SC.state_mismatches(out, want, check_next_pos=not want["done"]) == [], name
    slot = start["cur_num_gen"]
    assert toks[slot] == exp["token"], name
    assert toks[:slot] + toks[slot + 1:] == empty[1:], name
    assert bool(flag & 2) == exp["flag2"], name                 # argmax of the edited logits was EOS
    assert bool(flag & 1) == exp["tie"], name                   # the cut the oracle's sorted values show
    return False


def _run_table(V, eos, single_block, tiny_vocab):
    skipped = {False: [], True: []}
    total = {False: 0, True: 0}
    mixed = 0
    for cases in _launches(ALL):
        eng = _engine(cases[0]["cfg"], single_block, tiny_vocab)
        mixed += {SC.row_kind(c) for c in cases} == {"fast", "fallback", "done", "stalled"}
        exps, init, out, flags, toks = _one_step(eng, cases, V, eos)
        for b, c in enumerate(cases):
            total[c["top_p_variant"]] += 1
            if _check_row(c, exps[b], init[b], out[b], flags[b], toks[b], single_block):
                skipped[c["top_p_variant"]].append(c["name"])
    print(f"V={V} single_block={single_block}: {total[False]} + {total[True]} rows, skipped (stalled tie cuts) "
          f"{skipped[True]}; {mixed} launches mix all four kinds of row")
    assert mixed >= 2
    assert skipped[False] == []                                            # top_p = 1.0: zero skips
    assert len(skipped[True]) <= SC.MAX_TIE_FRACTION * total[True]
    return skipped


@pytest.mark.parametrize("path", ["fast_and_fallback", "single_block"])
def test_rules_one_step(path):
    """Every case at V = 65541: token, every state field (next_pos bitwise), the token buffer
    and flag bit 1, on the default path (multi-block fast kernel + single-block fallback) and
    on the single-block kernel alone. A row is skipped only when the device raised flag 4, the
    oracle's sorted values show a top-p cut inside a tie group, the path is the single-block one
    (on the default path the fast kernel resolves ties itself, and the table's seeds give the
    rows it hands to the single-block kernel no tie cut) and the row's state is untouched except
    done == 2; never with top_p = 1.0, and in at most a quarter of the top_p = 0.9 rows."""
    _run_table(V_BIG, EOS_BIG, path == "single_block", False)


def test_rules_small_vocab():
    """The same table at the tiny config's own V = 69 (token ids folded into range): the 16
    slices of the fast kernel hold 5 elements or none, fewer than k, so it takes its
    `i1 - i0 > k` shortcut; V and the leading dimension are odd. The oracle reports no tie
    cut at this V (asserted on the CPU), so nothing may be skipped. (A slice cannot overflow
    its 128 candidate slots here; that hand-over to the single-block kernel is case
    `slice_overflow` at V = 65541, ~650 tied candidates per slice.)"""
    skipped = _run_table(V_TINY, EOS_TINY, False, True)
    assert skipped[True] == []


def test_rules_fast_equals_single_block_philox():
    """Production noise (noise = NULL): the default path and the single-block kernel give
    identical tokens, states, token buffers and flags over the whole table."""
    n = 0
    for cases in _launches(ALL):
        res = []
        for single in (False, True):
            eng = _engine(cases[0]["cfg"], single, False)
            _, _, out, flags, toks = _one_step(eng, cases, V_BIG, EOS_BIG, reference_noise=False)
            res.append((out, flags, toks))
        (oa, fa, ta), (ob, fb, tb) = res
        for b, c in enumerate(cases):
            assert SC.state_mismatches(oa[b], _init_dict(ob[b])) == [], c["name"]
            assert ta[b] == tb[b], c["name"]
            if not c["state"]["done"]:
                assert not (fa[b] & 4) and fa[b] == fb[b], (c["name"], fa[b], fb[b])
                n += 1
    print(f"fast + fallback vs single-block, Philox noise: {n} rows identical")


@pytest.mark.parametrize("path", ["fast_and_fallback", "single_block"])
def test_silence_run_multi_step(path):
    """State carried on the device across 12 calls of t5g_sample_only, fresh logits per call
    that make silence token 8 dominant (10.0: no penalty up to a run of 3; at a run of 4 the
    penalty halves it, which takes it out of the top 30, so steps 0-4 give token 8 and step 5
    another token -- one step later if the rule were off by one). Rows 0-2 stop_repetition = 0, rows 3-5
    stop_repetition = 3, rows 6-7 a time budget that ends them at step 7 (config B:
    4 - 10 + 12.5 = 6.5 < 7). Every step's token, consec_silence, cur_num_gen and done equal
    the oracle loop; a finished row and its token buffer stay as they are."""
    steps, V, eos = 12, V_BIG, EOS_BIG
    eng = _engine("B", path == "single_block", False)
    cases = []
    for b in range(ROWS):
        row = dict(SC.ROW_DEFAULT, silence=True, stop_repetition=0 if b < 3 else 3)
        st = dict(SC.STATE_DEFAULT, cur_num_gen=0, current_length=20 + b, prompt_offset=10, est_total=300 + 7 * b,
                  first_input_len=50, target_total=4 if b >= 6 else -1)
        cases.append(dict(name=f"run{b}", row=row, state=st, cfg="B", ld_pad=12))
    from t5gemma_tts_amd.engine import reference_noise
    noise = torch.stack([reference_noise(400 + b, steps, V) for b in range(ROWS)])
    noise[:, :, 8] = SC.TINY_Q
    noise_dev = noise.contiguous().cuda()
    _setup(eng, cases, V, noise_dev, steps)
    state = [dict(c["state"]) for c in cases]
    want_toks = [[-1] * SC.MAX_GEN for _ in cases]
    g = torch.Generator().manual_seed(77)
    for s in range(steps):
        x = torch.randn(ROWS, V, generator=g) * 2.0
        x[:, 8] = 10.0
        lg = x.to(BF16)
        out, flags, toks = _sample(eng, ROWS, _upload_logits(list(lg), V, V + 12))
        for b, c in enumerate(cases):
            if not state[b]["done"]:
                tok, info = SC.oracle_step(lg[b], SC.oracle_params(c), SC.oracle_state(state[b]), noise[b, s], eos, "B")
                token, state[b], _ = SC.finish_step(state[b], tok, info, SC.SILENCE, eos, "B")
                want_toks[b][s] = token
                assert bool(flags[b] & 2) == (info["argmax"] == eos), (s, b)
            assert not flags[b] & 4, (s, b)
            assert SC.state_mismatches(out[b], state[b], check_next_pos=not state[b]["done"]) == [], (s, b)
            assert toks[b] == want_toks[b], (s, b)
    print(f"{path}: tokens {[t[:steps] for t in want_toks]}, final runs {[st['consec_silence'] for st in state]}")
    assert all(st["consec_silence"] == steps - 1 for st in state[:3])             # no penalty: the run goes on
    assert all(t[:5] == [8] * 5 and t[5] != 8 for t in want_toks[3:])             # the penalty at a run of 4
    assert all(st["done"] == 1 and st["cur_num_gen"] == 8 and t[7] == eos for st, t in zip(state[6:], want_toks[6:]))


def test_sampler_setup_rejects_out_of_list_rows():
    """t5g_sampler_setup checks every row's list ranges and prev_token on the host and returns
    T5G_EINVAL before any copy; the ranges that end exactly at the lists' ends pass."""
    from t5gemma_tts_amd import _lib
    eng = _engine("A", False, False)
    tk, ntk, sl, nsl = SC.shared_lists()

    def setup(row_kw=None, state_kw=None, n_tk=ntk, n_sl=nsl):
        rows = (_lib.SamplerRow * 2)()
        sts = (_lib.SamplerState * 2)()
        for b in range(2):
            rows[b] = _lib.SamplerRow(top_k=30, top_p=0.9, temperature=0.8)
            sts[b] = SC.lib_state(SC.STATE_DEFAULT)
        for k, v in (row_kw or {}).items():
            setattr(rows[1], k, v)
        for k, v in (state_kw or {}).items():
            setattr(sts[1], k, v)
        return eng.L.t5g_sampler_setup(eng.h, 2, rows, sts, tk, n_tk, sl, n_sl, None, 0, stream())

    einval = -1
    assert setup(dict(n_silence=3, silence_off=nsl - 2)) == einval          # silence range past the list
    assert setup(dict(n_silence=nsl + 1, silence_off=0)) == einval
    assert setup(dict(n_silence=1, silence_off=0), n_sl=0) == einval        # no list uploaded
    assert setup(dict(n_silence=1, silence_off=-1)) == einval               # negative offset / length
    assert setup(dict(n_silence=-1, silence_off=0)) == einval
    assert setup(dict(top_k_list_len=4, top_k_list_off=ntk - 3)) == einval  # top-k range past the list
    assert setup(dict(top_k_list_len=1, top_k_list_off=ntk)) == einval
    assert setup(dict(top_k_list_len=1, top_k_list_off=0), n_tk=0) == einval
    assert setup(dict(top_k_list_len=2, top_k_list_off=-2)) == einval
    assert setup(dict(top_k_list_len=-4, top_k_list_off=0)) == einval
    assert setup(state_kw=dict(prev_token=V_BIG)) == einval                 # prev_token indexes the logits
    assert setup(state_kw=dict(prev_token=1 << 30)) == einval
    # accepted: ranges that end at the lists' ends, the last token id, no previous token
    assert setup(dict(n_silence=3, silence_off=nsl - 3, top_k_list_len=4, top_k_list_off=ntk - 4),
                 dict(prev_token=V_BIG - 1)) == 0
    assert setup(state_kw=dict(prev_token=-1)) == 0
    torch.cuda.synchronize()

"""The host restatement of the sampler (t5g_host_sample, csrc/host_sampler.cpp) on every case
of tests/sampler_cases.py at the production vocabulary: token and every state field equal the
oracle's sample_helper extended with the capacity rules, the counters and next_pos
(sampler_cases.expected). The host function follows std::sort, so a top-p cut inside a tie
group is no excuse here: nothing is skipped.

A row that starts done or stalled is stepped with ``done`` cleared, which is how the engine
resumes a stalled row on the host (engine.py _run_parity); that such rows do not move on the
device is tests/test_gpu_sampler_rules.py's part.
"""
import ctypes as C

import pytest

from tests import sampler_cases as SC

V = 65541
EOS = 65539
ALL = SC.all_cases()


def _host_step(case, exp):
    from t5gemma_tts_amd import _lib
    L = _lib.lib()
    tk, _, sl, _ = SC.shared_lists()
    row = SC.lib_row(case)
    st = SC.lib_state(dict(case["state"], done=0))
    out = _lib.SamplerState()
    tok = C.c_int32(-7)
    lg, nz = exp["logits"].clone(), exp["noise"]
    cfg = SC.CFGS[case["cfg"]]
    rc = L.t5g_host_sample(C.c_void_p(lg.data_ptr()), V, C.byref(row), tk, sl, C.byref(st),
                           C.c_void_p(nz.data_ptr()), EOS, SC.EOS_GUARD, int(SC.ENCODEC_SR) * cfg["extra_cutoff"],
                           cfg["text_guard"], SC.PROGRESS_SCALE, SC.MAX_GEN, SC.KEY_BOUND, C.byref(out),
                           C.byref(tok))
    assert rc == 0
    return tok.value, out


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_host_sampler_follows_every_rule(case):
    exp = SC.expected(case, V, EOS, clear_done=True)
    tok, out = _host_step(case, exp)
    print(f"{case['name']}: rule {exp['rule']}, sampled {exp['sampled']}, token {exp['token']} (host {tok}), "
          f"tie cut {exp['tie']}")
    assert tok == exp["token"]
    assert SC.state_mismatches(out, exp["state"], check_next_pos=not exp["state"]["done"]) == []


def test_table_reaches_its_rules():
    """Every case is decided by the rule it is named for (derived from the oracle's outputs),
    each rule by at least one fast-path and one single-block row, and the two force-stop twins
    are what they claim: argmax EOS with another token sampled; EOS sampled under another argmax."""
    by_rule = {}
    for c in ALL:
        exp = SC.expected(c, V, EOS)
        assert exp["rule"] == c["rule"], (c["name"], exp["rule"])
        assert (c["rule"] == "none") == (SC.row_kind(c) in ("done", "stalled"))
        by_rule.setdefault(exp["rule"], []).append(c["name"])
    assert set(by_rule) == {"none", "sampled", "sampled_eos", "argmax_eos", "text_guard", "budget", "cap_gen", "cap_len"}
    byname = {c["name"]: c for c in ALL}
    a = SC.expected(byname["force_argmax_eos"], V, EOS)
    assert a["sampled"] != EOS and a["token"] == EOS and a["flag2"]
    b = SC.expected(byname["force_sampled_eos"], V, EOS)
    assert b["sampled"] == EOS and b["token"] == EOS and not b["flag2"]
    kinds = {SC.row_kind(c) for c in ALL}
    assert kinds == {"fast", "fallback", "done", "stalled"}


def test_boosted_tokens_give_the_cases_teeth():
    """The cases that tell a rule's two sides apart by one boosted token: it is sampled on one
    side and filtered out on the other."""
    byname = {c["name"]: c for c in ALL}

    def tok(name):
        return SC.expected(byname[name], V, EOS)["token"]

    # the penalty applies from a run of 4 (> stop_repetition = 3) on, and with the factor 2 there
    assert tok("sil_pos_c3") == 8 and tok("sil_pos_c4") != 8 and tok("sil_pos_c6") != 8
    assert tok("sil_neg_c3") == 8 and tok("sil_neg_c4") != 8 and tok("sil_neg_c6") != 8
    assert tok("sil_pos_c4_stays") == 8 and tok("sil_neg_c4_stays") == 8
    assert tok("sil_prev_not_listed") == 5 and tok("sil_stop_rep0") == 8 and tok("sil_no_list") == 8
    st = {n: SC.expected(byname[n], V, EOS)["state"]["consec_silence"] for n in byname}
    assert (st["sil_pos_c3"], st["sil_pos_c4"], st["sil_pos_c4_stays"], st["sil_stop_rep0"]) == (4, 0, 5, 7)
    assert st["sil_other_silence_token"] == 0 and st["sil_non_silence_token"] == 0 and st["cap_gen_silence"] == 0
    # the per-step top-k entries: rank 35 survives k = 40 and not k = 20, rank 10 not k = 3
    import torch
    for name, rank, inside in [("tk_L0_step0_k40", 35, True), ("tk_L0_step1_k20", 35, False),
                               ("tk_L3_step0_k40", 35, True), ("tk_L0_step2_k100", 80, True),
                               ("tk_L3_step2_k100", 80, True), ("tk_L3_step3_k3", 10, False),
                               ("tk_L3_step77_k3", 2, True), ("minp_09_flat_skipped", 35, False),
                               ("minp_1_ignored", 35, False)]:
        e = SC.expected(byname[name], V, EOS)
        x = e["logits"].float().clone()
        x[EOS] = -float("inf")
        boosted = int(torch.sort(x, descending=True, stable=True)[1][rank])
        assert (e["token"] == boosted) == inside, name


def test_min_p_cases_apply_the_filter_and_see_both_switches():
    """The min_p = 0.05 cases at both vocabularies, from the oracle's arithmetic alone: the filter
    applies (0 < survivors < V); the token that holds the tiny draw is the result exactly where
    it clears the threshold; and the two slips the cases are built for would change the token --
    min_p ignored, and min_p applied without switching top-k and top-p off."""
    import torch
    from oracle import t5g_oracle as O
    names = ["minp_005_peaky", "minp_b", "ld_even_minp", "minp_005_below"]
    for v, eos in ((V, EOS), (69, 67)):
        for c in [c for c in ALL if c["name"].split("@")[0] in names]:
            e, r = SC.expected(c, v, eos), c["row"]
            x = e["logits"] / r["temperature"]
            probs = torch.softmax(x, dim=-1)
            keep = probs >= r["min_p"]
            boosted = SC.MINP_TOKENS[3]
            want_in = "below" not in c["name"]
            assert int(keep.sum()) == (4 if want_in else 3) and bool(keep[boosted]) == want_in, c["name"]
            assert (e["token"] == boosted) == want_in, c["name"]

            def pick(y):
                return int(torch.argmax(torch.softmax(y, dim=-1) / e["noise"]))
            ignored = pick(O.top_k_top_p_filtering(x.clone(), top_k=r["top_k"], top_p=r["top_p"], min_p=0.0))
            unswitched = pick(O.top_k_top_p_filtering(x.masked_fill(~keep, -float("inf")), top_k=r["top_k"],
                                                      top_p=r["top_p"], min_p=0.0))
            assert ignored != e["token"], c["name"]
            if want_in:
                assert unswitched != e["token"], c["name"]


def test_slice_overflow_case_overflows_a_slice():
    """Case slice_overflow is there to make the fast kernel hand the row over: in each of its 16
    slices (csrc/sampler.hip: FS_NB slices of ceil(V / 16)) more values tie with the slice's
    30th largest than the 128 candidate slots (FS_CAP) hold."""
    import torch
    case = next(c for c in ALL if c["name"] == "slice_overflow")
    x = (SC.expected(case, V, EOS)["logits"].float() / case["row"]["temperature"]).to(torch.bfloat16).float()
    sl = (V + 15) // 16
    for s0 in range(0, V, sl):
        part = x[s0:s0 + sl]
        if part.numel() > 30:
            kth = torch.topk(part, 30)[0][-1]
            assert int((part >= kth).sum()) > 128


def test_top_p_tie_cuts_stay_within_bound():
    """The device tests may skip a single-block row whose top-p cut falls inside a tie group;
    the oracle alone reports such a cut in no case with top_p = 1.0 and in at most a quarter
    of the top_p = 0.9 cases, at both vocabularies the device tests use."""
    for v, eos in ((V, EOS), (69, 67)):
        p1 = [c["name"] for c in ALL if not c["top_p_variant"] and SC.expected(c, v, eos)["tie"]]
        assert p1 == []
        p09 = [c for c in ALL if c["top_p_variant"]]
        tied = [c["name"] for c in p09 if SC.expected(c, v, eos)["tie"]]
        print(f"V={v}: {len(tied)} of {len(p09)} top_p=0.9 cases cut inside a tie group: {tied}")
        # on the default path only the fast kernel may meet such a cut (it resolves it itself)
        assert all(SC.row_kind(c) == "fast" for c in p09 if c["name"] in tied)
        assert len(tied) <= SC.MAX_TIE_FRACTION * len(p09)

"""One table of sampler rule cases, shared by tests/test_sampler_rules_cpu.py (the host
restatement, csrc/host_sampler.cpp) and tests/test_gpu_sampler_rules.py (the two device
sampler paths, csrc/sampler.hip).

A case is a plain dict: sampler parameters (``row``), an initial row state (``state``), a
logits recipe, noise tweaks and the engine constants it needs (``cfg``). The expected result
of one step is ``oracle.t5g_oracle.sample_helper`` -- the plain torch restatement of the
reference's ``sample_helper`` -- on a clone of the bf16 logits with the same noise row,
extended in plain Python with what the oracle leaves to its caller (``expected``): the two
capacity rules, the counters, ``done``, ``next_pos`` and flag bit 1.

Every boundary appears on both sides. ``rule`` names what decides the token of the case;
``expected`` derives the same name from the oracle's own outputs and the CPU test asserts
that the two agree, so the table cannot drift into cases that no longer reach their rule.
"""
import ctypes as C
import math
import struct
from unittest import mock

import torch

from oracle import t5g_oracle as O

BF16 = torch.bfloat16

# engine constants shared by every case (tests/test_gpu_sampler_rules.py builds its engines
# with them; the CPU test passes them to t5g_host_sample)
MAX_GEN = 128            # generated-token slots per row
MAX_AUDIO = 256          # self-attention cache slots per row
KEY_BOUND = 240          # t5g_engine_set_audio_max: the call's key bound (second capacity rule)
PROGRESS_SCALE = 2000.0
ENCODEC_SR = 50.0        # eos_guard = 50 // 5 = 10
EOS_GUARD = 10
# A: the tiny config as it stands (budget_extra = 50 * 1.0, no text guard);
# B: text_guard_frames_per_token = 10, extra_cutoff = 0.25 (budget_extra = 12.5)
CFGS = {"A": dict(text_guard=0, extra_cutoff=1.0), "B": dict(text_guard=10, extra_cutoff=0.25)}

# shared device lists; every row reads them at a non-zero offset (a kernel that dropped the
# offset would read [60, 61, 7]: token 8 not a silence token; or top-k 5 at every step)
SILENCE = (7, 8, 9)
SILENCE_BUF = [60, 61] + list(SILENCE)
SILENCE_OFF = 2
TOPK_LISTS = {"L0": [40, 20, 100, 0], "L3": [40, 20, 100, 3]}
TOPK_BUF = [5, 5] + TOPK_LISTS["L0"] + TOPK_LISTS["L3"]
TOPK_OFF = {"L0": 2, "L3": 6}
FS_KMAX = 64             # csrc/t5g_kernels.h: largest top-k the multi-block fast path takes

ROW_DEFAULT = dict(top_k=30, top_k_list=None, top_p=1.0, min_p=0.0, temperature=0.8, stop_repetition=0,
                   silence=False, eos_disabled=0)
STATE_DEFAULT = dict(cur_num_gen=100, current_length=200, prompt_offset=1, target_total=-1, est_total=1000,
                     prev_token=-1, consec_silence=0, first_input_len=5, done=0, ambiguous_steps=0,
                     last_token=-1, next_pos=0.25)
STATE_FIELDS = tuple(STATE_DEFAULT)
TINY_Q = 2.0 ** -14      # an exponential draw so small that its token wins whenever it survives the filters
SIL_ROW = dict(stop_repetition=3, silence=True)
# min_p cases: the bulk sits at -14 +/- 2 (no mass), these tokens carry about these probabilities
# after the temperature (logit = 6 + T ln(p / p[0]))
MINP_TOKENS = (20, 21, 22, 23)
MINP_KEEP = (0.50, 0.30, 0.13, 0.07)
MINP_BELOW = (0.50, 0.30, 0.153, 0.047)

CASES = []


def _c(name, rule, row=None, state=None, logits=(), noise=(), cfg="A", ld_pad=12, p09=True, scale=2.0,
       shift=0.0, seed=None):
    CASES.append(dict(name=name, rule=rule, row=dict(ROW_DEFAULT, **(row or {})),
                      state=dict(STATE_DEFAULT, **(state or {})), logits=tuple(logits), noise=tuple(noise),
                      cfg=cfg, ld_pad=ld_pad, p09=p09, scale=scale, shift=shift,
                      seed=100 + len(CASES) if seed is None else seed))


EOS_TOP = (("eos_top",),)
# ---- eff_len == 0: EOS -> -1e9 (and the clamp of a negative length to 0); one key later EOS wins
_c("eff0_eq", "sampled", state=dict(current_length=50, prompt_offset=50), logits=EOS_TOP)
_c("eff0_clamp", "sampled", state=dict(current_length=40, prompt_offset=50), logits=EOS_TOP)
_c("eff1", "argmax_eos", state=dict(current_length=51, prompt_offset=50), logits=EOS_TOP)
_c("done1_row", "none", state=dict(done=1, last_token=17, cur_num_gen=20), logits=EOS_TOP)
# ---- eos_guard: cur_num_gen <= 10 -> EOS = -10000
_c("guard_eq", "sampled", state=dict(cur_num_gen=EOS_GUARD), logits=EOS_TOP)
_c("guard_gt", "argmax_eos", state=dict(cur_num_gen=EOS_GUARD + 1), logits=EOS_TOP)
_c("guard_eq_eosdis", "sampled", row=dict(eos_disabled=1), state=dict(cur_num_gen=EOS_GUARD), logits=EOS_TOP)
_c("guard_gt_eosdis", "sampled", row=dict(eos_disabled=1), state=dict(cur_num_gen=EOS_GUARD + 1), logits=EOS_TOP)
_c("tk_L0_step2_k100", "sampled", row=dict(top_k_list="L0"), state=dict(cur_num_gen=2),
   noise=(("rank", 80, TINY_Q),))
# ---- argmax == EOS force-stop and its twin
_c("force_argmax_eos", "argmax_eos", row=dict(top_k=30, top_p=1.0, temperature=1.0), logits=EOS_TOP,
   noise=(("eos", 16.0), ("rank", 1, TINY_Q)), p09=False)
_c("force_sampled_eos", "sampled_eos", row=dict(top_k=30, top_p=1.0, temperature=1.0),
   logits=(("eos_second",),), noise=(("eos", TINY_Q),), p09=False)
_c("stalled_row", "none", state=dict(done=2, last_token=3, cur_num_gen=31, consec_silence=2, prev_token=8),
   row=SIL_ROW)
# ---- text guard (config B): eff_len > max(1, first_input_len) * 10
_c("tguard_50", "sampled", cfg="B", state=dict(current_length=51, first_input_len=5))
_c("tguard_51", "text_guard", cfg="B", state=dict(current_length=52, first_input_len=5))
_c("tguard_fil0_10", "sampled", cfg="B", state=dict(current_length=11, first_input_len=0))
_c("tguard_fil0_11", "text_guard", cfg="B", state=dict(current_length=12, first_input_len=0))
_c("tguard_off", "sampled", cfg="A", state=dict(current_length=52, first_input_len=5))
# ---- time budget: cur_num_gen > target_total - prompt_offset + budget_extra
_c("budget_int_floor", "sampled", state=dict(cur_num_gen=80, target_total=31))         # 30 + 50.0
_c("budget_int_over", "budget", state=dict(cur_num_gen=81, target_total=31))
_c("budget_frac_floor", "sampled", cfg="B", state=dict(cur_num_gen=72, target_total=61, first_input_len=50))
_c("budget_frac_over", "budget", cfg="B", state=dict(cur_num_gen=73, target_total=61, first_input_len=50))
_c("budget_none", "sampled", state=dict(cur_num_gen=120, target_total=-1))
_c("done1_row_b", "none", cfg="B", state=dict(done=1, last_token=9))
_c("minp_b", "sampled", cfg="B", row=dict(min_p=0.05, top_k=3), state=dict(first_input_len=50), shift=-14.0,
   logits=(("probs", MINP_KEEP),), noise=(("tok", MINP_TOKENS[3], TINY_Q),))
# ---- capacity: the last generated-token slot, the key bound
_c("cap_gen_below", "sampled", state=dict(cur_num_gen=MAX_GEN - 2))
_c("cap_gen_at", "cap_gen", state=dict(cur_num_gen=MAX_GEN - 1))
_c("cap_len_below", "sampled", state=dict(current_length=KEY_BOUND - 1))
_c("cap_len_at", "cap_len", state=dict(current_length=KEY_BOUND))
# the capacity rule comes before the silence update: EOS is no silence token, the run ends
_c("cap_gen_silence", "cap_gen", row=SIL_ROW, state=dict(cur_num_gen=MAX_GEN - 1, prev_token=8, consec_silence=2),
   logits=(("set", 8, 12.0),), noise=(("tok", 8, TINY_Q),))
# ---- silence run: stop_repetition = 3, penalty factor consec - 2 only when consec > 3.
# The 30th largest of 65541 randn * 2 logits is ~6.6. A dominant logit 10 stays on top at a run
# of 3 (no penalty) and leaves the top 30 at a run of 4 (10 / 2 = 5) and of 6 (10 / 4): an
# off-by-one in `consec_silence > stop_repetition`, or a multiply, keeps it on top
for cs in (3, 4, 6):
    _c(f"sil_pos_c{cs}", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=cs),
       logits=(("set", 8, 10.0),), noise=(("tok", 8, TINY_Q),))
# all logits near -3 (30th largest ~ -2.3), token 8 at -1.3 -> -1.3 / -2.6 / -5.2: out of the
# top 30 from a run of 4 on; a wrong divide keeps it
for cs in (3, 4, 6):
    _c(f"sil_neg_c{cs}", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=cs), scale=0.2, shift=-3.0,
       logits=(("set", 8, -1.3),), noise=(("tok", 8, TINY_Q),))
_c("sil_prev_not_listed", "sampled", row=SIL_ROW, state=dict(prev_token=5, consec_silence=6),
   logits=(("set", 5, 12.0),), noise=(("tok", 5, TINY_Q),))
_c("sil_stop_rep0", "sampled", row=dict(stop_repetition=0, silence=True), state=dict(prev_token=8, consec_silence=6),
   logits=(("set", 8, 12.0),), noise=(("tok", 8, TINY_Q),))
_c("sil_other_silence_token", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=2),
   logits=(("set", 9, 12.0),), noise=(("tok", 9, TINY_Q),))
_c("sil_non_silence_token", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=2),
   logits=(("set", 5, 12.0),), noise=(("tok", 5, TINY_Q),))
_c("sil_no_list", "sampled", row=dict(stop_repetition=3, silence=False), state=dict(prev_token=8, consec_silence=6),
   logits=(("set", 8, 12.0),), noise=(("tok", 8, TINY_Q),))
# ---- per-step top-k list, read at min(len - 1, cur_num_gen); a boosted token just inside or
# outside the entry's k tells a wrong entry apart
_c("tk_L0_step0_k40", "sampled", row=dict(top_k_list="L0"), state=dict(cur_num_gen=0), noise=(("rank", 35, TINY_Q),))
_c("tk_L0_step1_k20", "sampled", row=dict(top_k_list="L0"), state=dict(cur_num_gen=1), noise=(("rank", 35, TINY_Q),))
_c("tk_L0_step3_k0", "sampled", row=dict(top_k_list="L0"), state=dict(cur_num_gen=3), noise=(("rank", 500, TINY_Q),),
   p09=False)
_c("tk_L0_step77_k0", "sampled", row=dict(top_k_list="L0"), state=dict(cur_num_gen=77),
   noise=(("rank", 500, TINY_Q),), logits=(("peaky",),))
_c("tk_L3_step0_k40", "sampled", row=dict(top_k_list="L3"), state=dict(cur_num_gen=0), noise=(("rank", 35, TINY_Q),))
_c("tk_L3_step2_k100", "sampled", row=dict(top_k_list="L3"), state=dict(cur_num_gen=2), noise=(("rank", 80, TINY_Q),))
_c("tk_L3_step3_k3", "sampled", row=dict(top_k_list="L3"), state=dict(cur_num_gen=3), noise=(("rank", 10, TINY_Q),))
_c("tk_L3_step77_k3", "sampled", row=dict(top_k_list="L3"), state=dict(cur_num_gen=77), noise=(("rank", 2, TINY_Q),))
# ---- min_p. Applied (MINP_KEEP): four tokens clear 0.05, the fourth (p ~ 0.07) holds the tiny
# draw; it ranks below top_k = 3 and past the top_p = 0.9 cut (0.5 + 0.3 + 0.13), so it is the
# token only if the filter both applies and switches top-k / top-p off
_c("minp_005_peaky", "sampled", row=dict(min_p=0.05, temperature=0.9, top_k=3), shift=-14.0,
   logits=(("probs", MINP_KEEP),), noise=(("tok", MINP_TOKENS[3], TINY_Q),))
_c("minp_09_flat_skipped", "sampled", row=dict(min_p=0.9, temperature=1.0), scale=0.01,
   noise=(("rank", 35, TINY_Q),))
_c("minp_0_ignored", "sampled", row=dict(min_p=0.0), noise=(("rank", 35, TINY_Q),))
_c("minp_1_ignored", "sampled", row=dict(min_p=1.0), noise=(("rank", 35, TINY_Q),))
# ---- temperature exactly 1 / not 1
_c("temp_1", "sampled", row=dict(temperature=1.0))
_c("temp_13", "sampled", row=dict(temperature=1.3))
# ---- next_pos in double: the clamp to progress_scale, max(1, est_total - 1), odd denominators
_c("pos_clamped", "sampled", state=dict(est_total=100))
_c("pos_est1", "sampled", state=dict(est_total=1))
_c("pos_997", "sampled", state=dict(est_total=997, current_length=131))
_c("pos_333", "sampled", state=dict(est_total=333, current_length=77))
# ---- a slice of the fast path with more candidates than it can hand off (heavy ties): the row
# is finished by the single-block kernel
_c("slice_overflow", "sampled", logits=(("round", 4.0),), p09=False)
# ---- even logits leading dimension (every case above runs with an odd one)
_c("ld_even_default", "sampled", ld_pad=11)
_c("ld_even_guard_gt", "argmax_eos", ld_pad=11, state=dict(cur_num_gen=EOS_GUARD + 1), logits=EOS_TOP)
_c("ld_even_sil_pos_c6", "sampled", ld_pad=11, row=SIL_ROW, state=dict(prev_token=8, consec_silence=6),
   logits=(("set", 8, 12.0),), noise=(("tok", 8, TINY_Q),))
_c("ld_even_k100", "sampled", ld_pad=11, row=dict(top_k=100), noise=(("rank", 80, TINY_Q),))
_c("ld_even_minp", "sampled", ld_pad=11, row=dict(min_p=0.05, top_k=3), shift=-14.0,
   logits=(("probs", MINP_KEEP),), noise=(("tok", MINP_TOKENS[3], TINY_Q),))
_c("ld_even_done", "none", ld_pad=11, state=dict(done=1))
_c("ld_even_stalled", "none", ld_pad=11, state=dict(done=2))
_c("ld_even_cap_len_at", "cap_len", ld_pad=11, state=dict(current_length=KEY_BOUND))
# ---- (appended, so that the cases above keep their seeds)
# min_p threshold: the fourth token (p ~ 0.047, just below 0.05) holds the tiny draw and is inside
# top_k = 30: it must be filtered out; without min_p it would be the token (top_p = 1.0 only: a
# 0.9 cut would drop it as well)
_c("minp_005_below", "sampled", row=dict(min_p=0.05, temperature=0.9), shift=-14.0,
   logits=(("probs", MINP_BELOW),), noise=(("tok", MINP_TOKENS[3], TINY_Q),), p09=False)
# the penalty's size at a run of 4: 15 / 2 and -0.75 * 2 stay in the top 30, a factor 3 would not
_c("sil_pos_c4_stays", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=4),
   logits=(("set", 8, 15.0),), noise=(("tok", 8, TINY_Q),))
_c("sil_neg_c4_stays", "sampled", row=SIL_ROW, state=dict(prev_token=8, consec_silence=4), scale=0.2, shift=-3.0,
   logits=(("set", 8, -0.75),), noise=(("tok", 8, TINY_Q),), p09=False)

# logits seeds of the top_p = 0.9 variants: chosen on the CPU so that the oracle's top-p cut
# falls inside a tie group in every sixth of the fast-path rows at V = 65541 (the fast kernel
# must resolve those itself) and in no other, at V = 65541 and at V = 69 -- at most a quarter
# (tests/test_sampler_rules_cpu.py asserts the bound)
P09_SEED = {
    "eff0_eq": 6001, "eff0_clamp": 6037, "eff1": 6074, "done1_row": 6111, "guard_eq": 6148, "guard_gt": 6187,
    "guard_eq_eosdis": 6222, "guard_gt_eosdis": 6259, "tk_L0_step2_k100": 6296, "stalled_row": 6333,
    "tguard_50": 6370, "tguard_51": 6411, "tguard_fil0_10": 6446, "tguard_fil0_11": 6481, "tguard_off": 6518,
    "budget_int_floor": 6559, "budget_int_over": 6593, "budget_frac_floor": 6630, "budget_frac_over": 6667,
    "budget_none": 6704, "done1_row_b": 6740, "minp_b": 6777, "cap_gen_below": 6814, "cap_gen_at": 6851,
    "cap_len_below": 6895, "cap_len_at": 6925, "cap_gen_silence": 7089, "sil_pos_c3": 7006, "sil_pos_c4": 7036,
    "sil_pos_c6": 7075, "sil_neg_c3": 7380, "sil_neg_c4": 7358, "sil_neg_c6": 7184, "sil_prev_not_listed": 7221,
    "sil_stop_rep0": 7258, "sil_other_silence_token": 7295, "sil_non_silence_token": 7332, "sil_no_list": 7369,
    "tk_L0_step0_k40": 7407, "tk_L0_step1_k20": 7443, "tk_L0_step77_k0": 7504, "tk_L3_step0_k40": 7519,
    "tk_L3_step2_k100": 7556, "tk_L3_step3_k3": 7591, "tk_L3_step77_k3": 7699, "minp_005_peaky": 7665,
    "minp_09_flat_skipped": 7703, "minp_0_ignored": 7739, "minp_1_ignored": 7776, "temp_1": 7813, "temp_13": 7851,
    "pos_clamped": 7888, "pos_est1": 7925, "pos_997": 7962, "pos_333": 7998, "ld_even_default": 8042,
    "ld_even_guard_gt": 8076, "ld_even_sil_pos_c6": 8114, "ld_even_k100": 8146, "ld_even_minp": 8183,
    "ld_even_done": 8220, "ld_even_stalled": 8257, "ld_even_cap_len_at": 8294,
    "sil_pos_c4_stays": 8369,
}
MAX_TIE_FRACTION = 0.25


def all_cases():
    """Every case with top_p = 1.0, then the top_p = 0.9 variants of those that make sense
    under a top-p cut (named ``<case>@p09``)."""
    out = [dict(c, top_p_variant=False) for c in CASES]
    for c in CASES:
        if c["p09"]:
            v = dict(c, name=c["name"] + "@p09", row=dict(c["row"], top_p=0.9), top_p_variant=True)
            v["seed"] = P09_SEED.get(c["name"], c["seed"] + 5000)
            out.append(v)
    return out


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _fold(i, V):
    return i if i < V - 5 else i % (V - 5)


def make_logits(case, V, eos):
    g = torch.Generator().manual_seed(case["seed"])
    x = torch.randn(V, generator=g) * case["scale"] + case["shift"]
    for op in case["logits"]:
        if op[0] == "peaky":
            x[torch.randint(0, V - 5, (5,), generator=g)] += 8.0
        elif op[0] == "round":
            x = (x / op[1]).round() * op[1]
        elif op[0] == "set":
            x[_fold(op[1], V)] = op[2]
        elif op[0] == "probs":
            for i, pr in zip(MINP_TOKENS, op[1]):
                x[i] = 6.0 + case["row"]["temperature"] * math.log(pr / op[1][0])
        elif op[0] == "eos_top":
            x[eos] = -100.0
            x[eos] = x.max() + 0.5
        elif op[0] == "eos_second":
            x[eos] = -100.0
            x[eos] = x.max() - 0.25
        else:
            raise ValueError(op)
    return x.to(BF16).contiguous()


def make_noise(case, V, eos, logits):
    """The row's exponential draws (what torch.multinomial draws on the CPU), then the case's
    tweaks: a tiny draw makes its token win whenever the filters keep it."""
    q = O.draw_noise(torch.Generator().manual_seed(7919 + case["seed"]), V)
    for op in case["noise"]:
        if op[0] == "tok":
            q[_fold(op[1], V)] = op[2]
        elif op[0] == "eos":
            q[eos] = op[1]
        elif op[0] == "rank":     # the token with the (r + 1)-th largest raw logit, EOS aside
            x = logits.float().clone()
            x[eos] = -float("inf")
            order = torch.sort(x, descending=True, stable=True)[1]
            q[int(order[min(op[1], V - 6)])] = op[2]
        else:
            raise ValueError(op)
    return q.contiguous()


def top_k_list_of(case):
    name = case["row"]["top_k_list"]
    return None if name is None else TOPK_LISTS[name]


def step_top_k(case):
    """The top-k the step uses (the list entry at min(len - 1, cur_num_gen), or the scalar)."""
    tk = top_k_list_of(case)
    return case["row"]["top_k"] if tk is None else tk[min(len(tk) - 1, case["state"]["cur_num_gen"])]


def row_kind(case):
    """done / stalled rows must not move; a fallback row is one sampler_fast_kernel hands to
    the single-block kernel by its parameters alone."""
    if case["state"]["done"] == 1:
        return "done"
    if case["state"]["done"] == 2:
        return "stalled"
    k = step_top_k(case)
    if 0.0 < case["row"]["min_p"] < 1.0 or k <= 0 or k > FS_KMAX:
        return "fallback"
    return "fast"


def shared_lists():
    """(top_k_list, n, silence, n) as ctypes int32 arrays: the buffers of t5g_sampler_setup."""
    tk = (C.c_int32 * len(TOPK_BUF))(*TOPK_BUF)
    sl = (C.c_int32 * len(SILENCE_BUF))(*SILENCE_BUF)
    return tk, len(TOPK_BUF), sl, len(SILENCE_BUF)


def lib_row(case, index=0):
    from t5gemma_tts_amd import _lib
    r, tk = case["row"], top_k_list_of(case)
    return _lib.SamplerRow(top_k=0 if tk else r["top_k"], top_k_list_len=len(tk) if tk else 0,
                           top_k_list_off=TOPK_OFF[r["top_k_list"]] if tk else 0, top_p=r["top_p"],
                           min_p=r["min_p"], temperature=r["temperature"], stop_repetition=r["stop_repetition"],
                           n_silence=len(SILENCE) if r["silence"] else 0,
                           silence_off=SILENCE_OFF if r["silence"] else 0, eos_disabled=r["eos_disabled"],
                           seed_lo=1000 + index, seed_hi=0)


def lib_state(state, V=None):
    from t5gemma_tts_amd import _lib
    s = dict(state)
    if V is not None:
        for k in ("prev_token", "last_token"):
            if s[k] >= 0:
                s[k] = _fold(s[k], V)
    return _lib.SamplerState(**s)


def lib_rows_states(cases, V):
    from t5gemma_tts_amd import _lib
    rows = (_lib.SamplerRow * len(cases))()
    sts = (_lib.SamplerState * len(cases))()
    for b, c in enumerate(cases):
        rows[b] = lib_row(c, b)
        sts[b] = lib_state(c["state"], V)
    return rows, sts


def oracle_params(case):
    r, tk = case["row"], top_k_list_of(case)
    return O.SamplerParams(top_k=list(tk) if tk else r["top_k"], top_p=r["top_p"], min_p=r["min_p"],
                           temperature=r["temperature"], stop_repetition=r["stop_repetition"],
                           silence_tokens=SILENCE if r["silence"] else (), eos_disabled=bool(r["eos_disabled"]))


def oracle_state(state):
    return O.RowState(cur_num_gen=state["cur_num_gen"], current_length=state["current_length"],
                      prompt_offset=state["prompt_offset"],
                      target_total=None if state["target_total"] < 0 else state["target_total"],
                      est_total=state["est_total"], prev_token=state["prev_token"],
                      consec_silence=state["consec_silence"], first_input_len=state["first_input_len"])


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# ----------------------------------------------------------------------------
# expected result
# ----------------------------------------------------------------------------
def top_p_cut_in_tie(x, top_k, top_p, min_p, filtering=None):
    """Whether the oracle's top-p cut falls inside a group of tied values, from its sorted
    values alone: s_logits[nkeep - 1] == s_logits[nkeep]. ``x`` is what sample_helper hands
    to top_k_top_p_filtering (edited, temperature-scaled logits); ``filtering``: the oracle's
    top_k_top_p_filtering itself where the module's name is patched (oracle_step)."""
    V = x.numel()
    if 0.0 < min_p < 1.0:
        probs = torch.softmax(x, dim=-1)
        if int((probs < min_p).sum()) < V:
            return False          # min_p applied: top-p is switched off
    if top_p >= 1.0:
        return False
    y = (filtering or O.top_k_top_p_filtering)(x.clone(), top_k=top_k, top_p=1.0, min_p=0.0)
    s = torch.sort(y, descending=True)[0]
    over = torch.cumsum(torch.softmax(s, dim=-1), dim=-1) > top_p
    if not bool(over.any()):
        return False
    nkeep = int(torch.nonzero(over)[0]) + 1
    return nkeep < V and bool(s[nkeep - 1] == s[nkeep]) and bool(s[nkeep - 1] > -float("inf"))


def oracle_step(logits, params, rstate, noise, eos, cfg):
    """sample_helper on a clone of the logits; also reports the tie state of its top-p cut."""
    seen = {}
    real = O.top_k_top_p_filtering

    def spy(x, top_k=0, top_p=1.0, min_p=0.0, **kw):
        seen["tie"] = top_p_cut_in_tie(x.clone(), top_k, top_p, min_p, filtering=real)
        return real(x, top_k=top_k, top_p=top_p, min_p=min_p, **kw)

    with mock.patch.object(O, "top_k_top_p_filtering", spy):
        token, info = O.sample_helper(logits.clone(), params, rstate, noise, eos=eos, encodec_sr=ENCODEC_SR,
                                      extra_cutoff=CFGS[cfg]["extra_cutoff"],
                                      text_guard_frames_per_token=CFGS[cfg]["text_guard"])
    info["tie"] = seen["tie"]
    return token, info


def finish_step(state, token, info, silence, eos, cfg, max_gen=MAX_GEN, max_len=KEY_BOUND):
    """What the oracle leaves to its caller, in plain Python: ``state`` is the row state before
    the step (dict), ``token`` / ``info`` the oracle's result, whose silence update is redone
    here when a capacity rule replaces the token (the rule comes before that update)."""
    st = dict(state)
    cap_gen = state["cur_num_gen"] + 1 >= max_gen
    cap_len = state["current_length"] >= max_len
    if cap_gen or cap_len:
        token = eos
    st["consec_silence"] = state["consec_silence"] + 1 if (token in silence and token == state["prev_token"]) else 0
    st["prev_token"] = token
    st["cur_num_gen"] += 1
    st["current_length"] += 1
    st["last_token"] = token
    st["done"] = 1 if token == eos else 0
    if not st["done"]:
        v = (st["current_length"] - 1) / max(1, st["est_total"] - 1) * PROGRESS_SCALE
        st["next_pos"] = struct.unpack("<f", struct.pack("<f", min(v, PROGRESS_SCALE)))[0]
    eff_len = max(0, state["current_length"] - state["prompt_offset"])
    tg = CFGS[cfg]["text_guard"]
    if info["sampled"] == eos:
        rule = "sampled_eos"
    elif info["argmax"] == eos:
        rule = "argmax_eos"
    elif tg > 0 and eff_len > max(1, state["first_input_len"]) * tg:
        rule = "text_guard"
    elif info["budget"]:
        rule = "budget"
    elif cap_gen:
        rule = "cap_gen"
    elif cap_len:
        rule = "cap_len"
    else:
        rule = "sampled"
    return token, st, rule


_EXPECTED = {}


def expected(case, V, eos, clear_done=False):
    """dict(token, state, flag2, tie, rule, sampled, logits, noise) of one step of ``case`` at
    vocabulary V. A row that starts done (1) or stalled (2) does not move: token None, state
    unchanged. ``clear_done``: the step as the host resumes a stalled row (done cleared).
    Computed once per (case, V) and shared: callers must not modify it."""
    clear_done = bool(clear_done and case["state"]["done"])
    key = (case["name"], V, eos, clear_done)
    if key in _EXPECTED:
        return _EXPECTED[key]
    logits = make_logits(case, V, eos)
    noise = make_noise(case, V, eos, logits)
    state = dict(case["state"])
    for k in ("prev_token", "last_token"):
        if state[k] >= 0:
            state[k] = _fold(state[k], V)
    if clear_done:
        state["done"] = 0
    if state["done"]:
        res = dict(token=None, state=state, flag2=None, tie=False, rule="none", sampled=None)
    else:
        rs = oracle_state(state)
        tok, info = oracle_step(logits, oracle_params(case), rs, noise, eos, case["cfg"])
        silence = SILENCE if case["row"]["silence"] else ()
        token, st, rule = finish_step(state, tok, info, silence, eos, case["cfg"])
        if token == tok:      # no capacity rule: the oracle's own silence update must agree
            assert (st["consec_silence"], st["prev_token"]) == (rs.consec_silence, rs.prev_token)
        res = dict(token=token, state=st, flag2=info["argmax"] == eos, tie=info["tie"], rule=rule,
                   sampled=info["sampled"])
    res.update(logits=logits, noise=noise)
    _EXPECTED[key] = res
    return res


def state_mismatches(got, want, check_next_pos=True):
    """Fields of a _lib.SamplerState that differ from the expected dict (next_pos bitwise)."""
    bad = []
    for f in STATE_FIELDS:
        g = getattr(got, f)
        if f == "next_pos":
            if check_next_pos and f32_bits(g) != f32_bits(want[f]):
                bad.append((f, g, want[f]))
        elif g != want[f]:
            bad.append((f, g, want[f]))
    return bad

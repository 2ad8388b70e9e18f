"""Full-depth parity at the headline workload (BASELINE configs[2], C3): T5Gemma-TTS-2b-2b
(26 + 26 layers, d 2304, 8 x 256 heads, FFN 9216, V 65 541), a batch of 8 voice-clone rows
(T_x 60, T_p 151) on the GPU engine.

``test_c3_batch8_exact_vs_reference`` (parity mode, exact-order kernels): rows 0 and 5 are
the two ``golden_long`` utterances -- the reference's own ``inference_tts`` (models/
t5gemma.py, identical to hf_export/modeling_t5gemma_voice.py:565-862) run in the build
container to the full 751-token budget (L up to 903) -- inside a batch of 8; their tokens
and the sha of every step's full logit row must equal the reference's. Bitwise, no
tolerance.

``test_c3_full_depth_batch8_vs_reference`` (the FAST kernels, reference RNG stream): the
production kernels are not order-exact by design; against ``golden_full`` and the CPU
oracle teacher-forced on the GPU's token history they must agree within ``RTOL`` of max
|logit|, with equal top-30 candidate sets up to ties within that tolerance, and the
reference sampler fed the GPU's logits (and the same noise) must return the GPU's token.
Match rates are written to gpurun_out/parity_full.json."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from tests.engine_cases import load_golden, need_gpu, topk_agree

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
RTOL = 0.03        # teacher-forced max |gpu - ref| / max |ref| per step (26+26 bf16 layers)
TOPK = 30


def _long_rows(cfg, n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        x = rng.integers(3, cfg.backbone.text_vocab_size - 1, size=60)
        x[28] = cfg.x_sep_token
        y = rng.integers(0, cfg.audio_vocab_size, size=150).tolist() + [cfg.y_sep_token]
        rows.append(dict(x=[int(v) for v in x], y=[int(v) for v in y], tgt=len(y) + 500))
    return rows


def _write(name, payload):
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    with open(os.path.join(REPO, "gpurun_out", name), "w") as f:
        json.dump(payload, f, indent=1)


@pytest.mark.timeout(1200)
def test_c3_full_depth_batch8_vs_reference():
    need_gpu()
    from oracle.t5g_oracle import SamplerParams as OP
    from oracle.t5g_oracle import T5GemmaTTSOracle, draw_noise, sample_helper
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import state_dict_digest, synthetic_weights

    meta, arrs = load_golden("golden_full")
    cfg = named_config(meta["config"], **meta["config_kw"])
    sd = synthetic_weights(cfg, meta["weight_seed"])
    assert state_dict_digest(sd) == meta["weight_sha256"], "weights differ from the golden run"
    cases = meta["cases"]
    golden_rows = {0: 0, 5: 1}             # batch row -> golden case
    longs = _long_rows(cfg, 6, seed=20251226)
    utts, seeds, ocases = [], [], []
    li = 0
    for b in range(8):
        if b in golden_rows:
            c = cases[golden_rows[b]]
            utts.append(Utterance(x=c["x"], y=c["y"], tgt_y_len=c["tgt"]))
            seeds.append(c["seed"])
        else:
            r = longs[li]
            li += 1
            utts.append(Utterance(x=r["x"], y=r["y"], tgt_y_len=r["tgt"]))
            seeds.append(3000 + b)
    p = dict(top_k=30, top_p=0.9, min_p=0.0, temperature=0.8, stop_repetition=3, silence_tokens=())
    eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=8, max_text=64, max_audio=151 + 1 + 520,
                           max_gen=520)
    out = eng.generate(utts, SamplingParams(**p), seeds=seeds, parity=True, exact=False, record_logits=True)
    logits = out["logits"]                 # per step: [8, V] on device
    from t5gemma_tts_amd import _lib
    report = {"rtol": RTOL, "rows": {}, "source_digest": _lib.kernel_source_digest("fast_path")}
    orc = T5GemmaTTSOracle(cfg, sd)
    op = OP(**p)

    def teacher_forced(b, max_steps=None):
        u = utts[b]
        ctx = orc.prepare(u.x, u.y, u.tgt_y_len)
        st = ctx["state"]
        gen = torch.Generator().manual_seed(int(seeds[b]))
        toks = out["gen"][b].tolist()
        worst, exact_rows, topk_ok, ref_tok_same, n = 0.0, 0, 0, 0, 0
        for t, tok in enumerate(toks):
            if max_steps is not None and t >= max_steps:
                break
            lo = orc.step_logits(ctx)
            lg = logits[t][b].cpu()
            noise = draw_noise(gen, lo.shape[-1])
            scale = lo.float().abs().max().item()
            err = (lg.float() - lo.float()).abs().max().item() / max(scale, 1e-6)
            worst = max(worst, err)
            exact_rows += int(torch.equal(lg, lo))
            topk_ok += int(topk_agree(lg, lo, TOPK, RTOL * scale))
            st_g, st_r = copy.deepcopy(st), copy.deepcopy(st)
            tok_g, _ = sample_helper(lg.clone(), op, st_g, noise, eos=cfg.eog_inference, encodec_sr=cfg.encodec_sr,
                                     extra_cutoff=cfg.extra_cutoff)
            tok_r, _ = sample_helper(lo.clone(), op, st_r, noise, eos=cfg.eog_inference, encodec_sr=cfg.encodec_sr,
                                     extra_cutoff=cfg.extra_cutoff)
            assert tok_g == tok, f"row {b} step {t}: reference sampler on GPU logits -> {tok_g}, GPU {tok}"
            ref_tok_same += int(tok_r == tok)
            n += 1
            ctx["state"] = st = st_g
            st.cur_num_gen += 1
            st.current_length += 1
            if tok == cfg.eog_inference:
                break
            orc.advance(ctx, tok)
        return dict(steps=n, max_rel_err=worst, bit_identical_rows=exact_rows, topk_agree=topk_ok,
                    ref_sampler_same_token=ref_tok_same, kv_len_max=len(utts[b].y) + 1 + n)

    # golden rows: free-running vs the reference's tokens + teacher-forced vs the oracle
    for b, ci in golden_rows.items():
        c = cases[ci]
        g = out["gen"][b].tolist()
        prefix = 0
        while prefix < min(len(g), len(c["gen"])) and g[prefix] == c["gen"][prefix]:
            prefix += 1
        top_idx, top_val = arrs[f"top_idx_{ci}"], torch.from_numpy(arrs[f"top_vals_{ci}"].astype(np.int16)).view(BF16)
        gold_ok = 0
        for t in range(min(prefix + 1, len(g), top_idx.shape[0])):   # same history up to step t
            lg = logits[t][b].cpu()
            ref_v = top_val[t].float()
            got_v = lg[torch.from_numpy(top_idx[t]).long()].float()
            scale = ref_v.abs().max().item()
            assert (got_v - ref_v).abs().max().item() <= RTOL * scale, (b, t)
            gv, gi = torch.topk(lg.float(), TOPK)
            gset = set(gi.tolist())
            rset = {int(i) for i, v in zip(top_idx[t][:TOPK], ref_v[:TOPK]) if v.item() > ref_v[TOPK - 1].item()
                    + RTOL * scale}
            gold_ok += int(rset <= gset)
        tf = teacher_forced(b)
        tf.update(golden_tokens_exact=g == c["gen"], golden_prefix_match=prefix, golden_steps=len(c["gen"]),
                  golden_topk_agree=gold_ok)
        report["rows"][f"golden_{ci}"] = tf
        assert tf["max_rel_err"] <= RTOL and tf["topk_agree"] == tf["steps"], tf
    # one long row, every step teacher-forced (attention over 152 .. 667 keys)
    tf = teacher_forced(1)
    report["rows"]["long_row1"] = tf
    assert tf["steps"] > 400 and tf["max_rel_err"] <= RTOL, tf
    assert tf["topk_agree"] >= tf["steps"] - 2, tf
    # the other long rows: the reference sampler on the GPU's logits reproduces every token
    from oracle.t5g_oracle import RowState
    for b in (2, 3, 4, 6, 7):
        u = utts[b]
        st = RowState(current_length=len(u.y) + 1, prompt_offset=len(u.y) + 1, target_total=u.tgt_y_len,
                      first_input_len=len(u.x))
        st.est_total = u.tgt_y_len + 1
        gen = torch.Generator().manual_seed(int(seeds[b]))
        toks = out["gen"][b].tolist()
        for t, tok in enumerate(toks):
            noise = draw_noise(gen, cfg.n_audio_tokens)
            tok_g, _ = sample_helper(logits[t][b].cpu().clone(), op, st, noise, eos=cfg.eog_inference,
                                     encodec_sr=cfg.encodec_sr, extra_cutoff=cfg.extra_cutoff)
            assert tok_g == tok, (b, t)
            st.cur_num_gen += 1
            st.current_length += 1
        report["rows"][f"long_row{b}"] = {"steps": len(toks), "sampler_exact": True}
    _write("parity_full.json", report)
    print(json.dumps(report))


@pytest.mark.timeout(900)
def test_c3_batch8_exact_vs_reference():
    need_gpu()
    import hashlib
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import state_dict_digest, synthetic_weights
    with open(os.path.join(GOLDEN, "golden_long.json")) as f:
        meta = json.load(f)
    cfg = named_config(meta["config"], **meta["config_kw"])
    sd = synthetic_weights(cfg, meta["weight_seed"])
    assert state_dict_digest(sd) == meta["weight_sha256"]
    cases = meta["cases"]
    golden_rows = {0: 0, 5: 1}
    longs = _long_rows(cfg, 6, seed=7)
    utts, seeds, li = [], [], 0
    for b in range(8):
        if b in golden_rows:
            c = cases[golden_rows[b]]
            utts.append(Utterance(x=c["x"], y=c["y"], tgt_y_len=c["tgt"]))
            seeds.append(c["seed"])
        else:
            r = longs[li]
            li += 1
            utts.append(Utterance(x=r["x"], y=r["y"], tgt_y_len=r["tgt"]))
            seeds.append(4000 + b)
    p = SamplingParams(top_k=30, top_p=0.9, min_p=0.0, temperature=0.8, stop_repetition=3)
    eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=8, max_text=64, max_audio=1024, max_gen=760)
    out = eng.generate(utts, p, seeds=seeds, parity=True, record_logits=True)
    report = {}
    for b, ci in golden_rows.items():
        c = cases[ci]
        n = len(c["gen"])
        shas = [hashlib.sha256(lg[b].cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:16]
                for lg in out["logits"][:n]]
        eq = sum(a == e for a, e in zip(shas, c["logit_sha"]))
        report[f"golden_long_{ci}"] = {"steps": n, "tokens_equal": out["gen"][b].tolist() == c["gen"],
                                       "logit_rows_equal": eq}
    _write("parity_full_exact.json", report)
    print(json.dumps(report))
    for r in report.values():
        assert r["tokens_equal"] and r["logit_rows_equal"] == r["steps"], report


# (golden, batch, golden row's slot): the reference's full-depth runs of BASELINE rows
# (tests/golden/make_golden.py gen_config_goldens), each alone and inside a batch of the
# workload's own size (the other rows: bench.make_batch rows of the same shape)
CONFIG_GOLDENS = [("golden_c2", 1, 0), ("golden_c1", 1, 0), ("golden_c4", 8, 3), ("golden_c2", 32, 17),
                  ("golden_longprompt", 1, 0), ("golden_longprompt", 4, 2), ("golden_longprompt2k", 1, 0),
                  # the reference CLI's longest prompt (cut_off_sec 100: 5 001 codes, a 5 003-token
                  # prefill) with a 90 s target (estimated length 9 503)
                  ("golden_longprompt5k", 1, 0)]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,batch,slot", CONFIG_GOLDENS)
def test_config_golden_exact(name, batch, slot):
    """Parity mode == the reference's own generate on BASELINE rows run to their full
    budget: every token and every step's logits row (sha of the bf16 bits), bitwise."""
    need_gpu()
    import hashlib
    import sys
    sys.path.insert(0, REPO)
    from bench import make_batch
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import state_dict_digest, synthetic_weights
    path = os.path.join(GOLDEN, name + ".json")
    if not os.path.exists(path):
        pytest.fail(f"{name} not generated (tests/golden/make_golden.py --only {name[7:]})")
    with open(path) as f:
        meta = json.load(f)
    cfg = named_config(meta["config"], **meta["config_kw"])
    sd = synthetic_weights(cfg, meta["weight_seed"])
    assert state_dict_digest(sd) == meta["weight_sha256"]
    c = meta["cases"][0]
    others = make_batch(cfg, batch, seed=3131, T_x=len(c["x"]), T_p=max(len(c["y"]) - 1, 0))
    utts, seeds = [], []
    for b in range(batch):
        if b == slot:
            utts.append(Utterance(x=c["x"], y=c["y"], tgt_y_len=c["tgt"]))
            seeds.append(c["seed"])
        else:
            x, y, tgt = others[b]
            # the other rows end no later than the golden row's budget allows for
            utts.append(Utterance(x=x, y=y, tgt_y_len=min(tgt, len(y) + 1 + max(c["tgt"] - len(c["y"]), 16))))
            seeds.append(5000 + b)
    p = SamplingParams(top_k=c["top_k"], top_p=c["top_p"], min_p=c["min_p"], temperature=c["temperature"],
                       stop_repetition=c["stop_repetition"])
    eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=batch, max_text=64,
                           max_audio=max(1024, len(c["y"]) + len(c["gen"]) + 16),
                           max_gen=max(760, len(c["gen"]) + 8))
    out = eng.generate(utts, p, seeds=seeds, parity=True, record_logits=True)
    n = len(c["gen"])
    shas = [hashlib.sha256(lg[slot].cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:16]
            for lg in out["logits"][:n]]
    eq = [a == e for a, e in zip(shas, c["logit_sha"])]
    first_bad = eq.index(False) if not all(eq) else None
    rep = {"name": name, "batch": batch, "steps": n, "tokens_equal": out["gen"][slot].tolist() == c["gen"],
           "logit_rows_equal": sum(eq), "first_differing_step": first_bad}
    _write(f"parity_{name}_b{batch}.json", rep)
    print(json.dumps(rep))
    assert rep["tokens_equal"] and rep["logit_rows_equal"] == n, rep


@pytest.mark.timeout(600)
def test_sliding_window_long_prompt_golden():
    """golden_longprompt4k: a 4 100-code prompt (a 4 101-token prefill, past the 2b-2b
    sliding layers' 4 096-key window: the explicit prefill mask, then the
    DynamicSlidingWindowLayer trim at every decode step) and 8 steps, against the reference's
    own run: every token and every logits row bitwise. (Round 4 had steps 1-2 one bf16 ulp
    off: one element of layer 24's prefill attention sat on a bf16 tie that aten broke with
    glibc's expf, not the correctly rounded exp -- tools/dbg/dbg_window_kv.py and
    tools/cpu_order/diag_layer_row.py localised it)"""
    need_gpu()
    import hashlib
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import state_dict_digest, synthetic_weights
    with open(os.path.join(GOLDEN, "golden_longprompt4k.json")) as f:
        meta = json.load(f)
    z = np.load(os.path.join(GOLDEN, "golden_longprompt4k.npz"))
    cfg = named_config(meta["config"], **meta["config_kw"])
    assert cfg.backbone.sliding_window == 4096
    sd = synthetic_weights(cfg, meta["weight_seed"])
    assert state_dict_digest(sd) == meta["weight_sha256"]
    c = meta["cases"][0]
    assert len(c["y"]) + 1 > cfg.backbone.sliding_window
    p = SamplingParams(top_k=c["top_k"], top_p=c["top_p"], min_p=c["min_p"], temperature=c["temperature"],
                       stop_repetition=c["stop_repetition"])
    eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=1, max_text=64,
                           max_audio=len(c["y"]) + len(c["gen"]) + 16, max_gen=len(c["gen"]) + 8)
    out = eng.generate([Utterance(x=c["x"], y=c["y"], tgt_y_len=c["tgt"])], p, seeds=[c["seed"]], parity=True,
                       record_logits=True)
    rows = []
    for s_, lg in enumerate(out["logits"][:len(c["gen"])]):
        bits = lg[0].cpu().view(torch.int16).numpy()
        d = np.abs(bits[z["top_idx_0"][s_]].astype(np.int32) - z["top_vals_0"][s_].astype(np.int32))
        rows.append((hashlib.sha256(bits.tobytes()).hexdigest()[:16] == c["logit_sha"][s_], int(d.max())))
    rep = {"tokens_equal": out["gen"][0].tolist() == c["gen"], "rows_bitwise": sum(r[0] for r in rows),
           "of": len(rows), "max_top64_ulps": max(r[1] for r in rows)}
    _write("parity_golden_longprompt4k_b1.json", rep)
    print(json.dumps(rep))
    assert rep["tokens_equal"] and rep["rows_bitwise"] == rep["of"], rep
    # the fast path serves the same 4 101-token prompt (its decode attention covers up to
    # 192 chunks of 64 keys) and stops at the same budget
    fast = eng.generate([Utterance(x=c["x"], y=c["y"], tgt_y_len=c["tgt"])], p, seeds=[c["seed"]])
    assert len(fast["gen"][0]) == len(c["gen"]) and fast["gen"][0][-1].item() == cfg.eog_inference


@pytest.mark.timeout(600)
def test_fast_path_capacity_is_per_call():
    """the fast path's capacity is the call's, not the engine's. An engine
    sized for the reference's longest request (12 288 keys: a 100 s prompt + the 120 s
    duration cap) serves a C3 batch of 8 (T_x 60, T_p 151, 751 tokens per row) on the fast
    kernels with tokens identical to an engine of 1 024 keys (the decode grids and the stop
    rule follow the call's key bound, t5g_engine_set_audio_max)."""
    need_gpu()
    import bench
    from t5gemma_tts_amd.config import named_config
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import synthetic_weights
    cfg = named_config("2b2b", extra_cutoff=5.0)
    sd = synthetic_weights(cfg, 13, device="cuda")
    rows = bench.make_batch(cfg, 8, seed=20251226)
    utts = [Utterance(x=x, y=y, tgt_y_len=t) for x, y, t in rows]
    p = SamplingParams(top_k=30, top_p=0.9, temperature=0.8, eos_disabled=True)
    outs = []
    for cap in (1024, 12288):
        eng = T5GemmaTTSEngine(cfg, sd, device="cuda:0", max_batch=8, max_text=64, max_audio=cap, max_gen=800)
        outs.append(eng.generate(utts, p, seeds=list(range(100, 108))))
        eng.close()
        del eng
        torch.cuda.empty_cache()
    for b in range(8):
        assert len(outs[0]["gen"][b]) == 751
        assert torch.equal(outs[0]["gen"][b], outs[1]["gen"][b]), b

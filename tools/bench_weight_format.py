"""A/B of the decode weight formats on one of bench.py's workloads (default C3: 8 rows, T_x 60,
T_p 151, 751 tokens per row): one process, one session, the arms interleaved round after round --

    bf16          the default engine (whole-layer launches)
    fp8           weight_format="fp8" (per-op launches on the P8 GEMVs, P8 head)
    bf16_per_op   the default engine after set_fused(False): the same launches as fp8, on bf16
    fp8_block     the fp8 engine after set_fp8_block(True): whole-layer launches on the P8 images
    fp8_mlp       the fp8 engine after set_fp8_mlp(True) alone: the MLP-half launch on the P8 images

(``--arms``, a comma list; default the first four, on ``--workload c5`` -- 32 rows, where a bf16
engine runs the MLP-half launch -- bf16, fp8 and fp8_mlp)
each ``--steps`` timed generate() calls after ``--warmup`` untimed ones, as bench.py times
them (the workload definitions are bench.py's own, imported). One JSON line per run goes to
``--out`` (default profiles/r12_fp8_block_c3_ab.jsonl, on c5 profiles/r13_fp8_mlp_c5_ab.jsonl), then a summary line: tok/s per run, the
within-arm spread over the rounds, and the device time of one decode step (t5g_time_decode_step)
per arm. The arms that take the whole-layer launch also record the launch alone
(t5g_time_decode_layer: ``decode_layer_us`` with stage S where the step runs it,
``decode_layer_front_us`` after set_attn_in_block(1)), the launch's algorithmic bytes in the
arm's format (``_lib.fused_block_bytes``) and with them its fraction of the 8 TB/s HBM peak.
The fp8_mlp arm, and the bf16 arm past 16 rows, record the MLP-half launch alone
(t5g_time_decode_mlp at the workload's row count: ``decode_mlp_us``) with its algorithmic bytes
(``_lib.fused_mlp_bytes``).
The baseline of any statement about fp8 or fp8_block is the bf16 runs of the same file.

    python tools/bench_weight_format.py --rounds 2 --steps 20 --warmup 5
    python tools/bench_weight_format.py --workload c5 --rounds 2 --steps 6 --warmup 2
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (WORKLOADS, request_rows, request_seed, DUR_FRAMES)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--workload", choices=sorted(bench.WORKLOADS), default="c3")
    ap.add_argument("--time-iters", type=int, default=200, help="decode steps timed by t5g_time_decode_step")
    ap.add_argument("--arms", default="", help="comma list of arms (default: by workload, see above)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    known = ["bf16", "fp8", "bf16_per_op", "fp8_block", "fp8_mlp"]
    arms = args.arms.split(",") if args.arms else ["bf16", "fp8", "fp8_mlp"] if args.workload == "c5" else known[:4]
    if not arms or any(a not in known for a in arms):
        ap.error(f"--arms: a comma list of {known}")
    if not args.out:
        args.out = os.path.join(REPO, "profiles", "r13_fp8_mlp_c5_ab.jsonl" if args.workload == "c5"
                                else "r12_fp8_block_c3_ab.jsonl")

    import torch

    from t5gemma_tts_amd import _lib
    from t5gemma_tts_amd.config import config_2b2b
    from t5gemma_tts_amd.engine import SamplingParams, T5GemmaTTSEngine, Utterance
    from t5gemma_tts_amd.weights import synthetic_weights

    B, T_x, T_p, _, _ = bench.WORKLOADS[args.workload]
    dev = "cuda:0"
    cfg = config_2b2b()
    torch.manual_seed(1234)
    sd = synthetic_weights(cfg, seed=1234, device=dev)
    n_tok_row = bench.DUR_FRAMES + int(cfg.extra_budget) + 1
    kw = dict(device=dev, max_batch=B, max_text=128, max_audio=T_p + 1 + n_tok_row + 8, max_gen=n_tok_row + 4)
    engines = {}
    if any(not a.startswith("fp8") for a in arms):
        engines["bf16"] = T5GemmaTTSEngine(cfg, sd, **kw)
    if any(a.startswith("fp8") for a in arms):
        engines["fp8"] = T5GemmaTTSEngine(cfg, sd, weight_format="fp8", **kw)
    rows = bench.request_rows(cfg, B, T_x, T_p)
    utts = [Utterance(x=r[3:3 + r[0]], y=r[3 + r[0]:], tgt_y_len=r[1]) for r in rows]
    params = SamplingParams(top_k=30, top_p=0.9, temperature=0.8, stop_repetition=3, eos_disabled=True)
    bb = cfg.backbone
    shape = dict(d=bb.hidden_size, f=bb.intermediate_size, q_dim=bb.num_attention_heads * bb.head_dim,
                 kv_dim=bb.num_key_value_heads * bb.head_dim, n_layers=bb.num_decoder_layers)

    def layer_launch(eng, stream, mode: int) -> dict:
        """The whole-layer launch alone (208 launches rotated over the layers, as bench.py's
        roofline leg), with stage S placed by set_attn_in_block(mode)."""
        us, keys = C.c_float(), C.c_float()
        eng.set_attn_in_block(mode)
        try:
            _lib.check(eng.L.t5g_time_decode_layer(eng.h, B, 208, stream, C.byref(us), C.byref(keys)),
                       "time_decode_layer")
        finally:
            eng.set_attn_in_block(2)
        nbytes = _lib.fused_block_bytes(B, T_x, self_keys=keys.value, weight_format=eng.weight_format, **shape)
        return {"us": round(us.value, 2), "keys": round(keys.value, 1), "bytes": round(nbytes),
                "hbm_peak_fraction": round(nbytes / (us.value * 1e-6) / 8e12, 4)}

    def run(arm: str, rnd: int) -> dict:
        eng = engines["fp8" if arm.startswith("fp8") else "bf16"]
        eng.set_fused(arm != "bf16_per_op")
        if eng.weight_format == "fp8":
            eng.set_fp8_block(arm == "fp8_block")
            eng.set_fp8_mlp(arm == "fp8_mlp")
        m0 = eng.mlp_half_launches()
        step = lambda i: sum(len(g) for g in eng.generate(   # noqa: E731
            utts, params, seeds=[bench.request_seed(i, r[2]) for r in rows], chunk=64)["gen"])
        for i in range(args.warmup):
            step(i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tokens = sum(step(100 + i) for i in range(args.steps))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        # device time of one decode step (sampler excluded) at the cache lengths the call left
        us = C.c_float()
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(eng.L.t5g_time_decode_step(eng.h, args.time_iters, stream, C.byref(us)), "time_decode_step")
        out = {}
        if arm == "fp8_mlp" or (arm == "bf16" and B > 16):
            mus = C.c_float()
            _lib.check(eng.L.t5g_time_decode_mlp(eng.h, B, 208, stream, C.byref(mus)), "time_decode_mlp")
            nbytes = _lib.fused_mlp_bytes(B, shape["d"], shape["f"], weight_format=eng.weight_format)
            out = {"decode_mlp_us": round(mus.value, 2), "fused_mlp_bytes": nbytes,
                   "decode_mlp_hbm_peak_fraction": round(nbytes / (mus.value * 1e-6) / 8e12, 4)}
        if arm in ("bf16", "fp8_block") and B <= 16:
            tail, front = layer_launch(eng, stream, 2), layer_launch(eng, stream, 1)
            out = {**out, "decode_layer_us": tail["us"], "decode_layer_front_us": front["us"],
                   "fused_block_bytes": tail["bytes"], "decode_layer_keys": tail["keys"],
                   "decode_layer_hbm_peak_fraction": tail["hbm_peak_fraction"],
                   "decode_layer_front_hbm_peak_fraction": front["hbm_peak_fraction"]}
        eng.set_fused(True)
        if eng.weight_format == "fp8":
            eng.set_fp8_block(False)
            eng.set_fp8_mlp(False)
        return {**out, "arm": arm, "round": rnd, "workload": args.workload, "steps": args.steps, "warmup": args.warmup,
                "tokens": tokens, "seconds": round(dt, 4), "tok_s": round(tokens / dt, 1),
                "generate_ms_per_step": round(1e3 * dt / args.steps, 2),
                "mlp_half_launches": eng.mlp_half_launches() - m0,
                "decode_step_us": round(us.value, 1), "weight_format": eng.native_weight_format(),
                "block_launches": eng.block_launches(), "device": torch.cuda.get_device_name(0)}

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    runs = []
    with open(args.out, "w") as f:
        for rnd in range(args.rounds):
            for arm in arms:
                r = run(arm, rnd)
                runs.append(r)
                f.write(json.dumps(r) + "\n")
                f.flush()
                print(json.dumps(r), flush=True)
        summary = {"summary": True, "weights": "synthetic (seed 1234)"}
        for arm in arms:
            v = [r["tok_s"] for r in runs if r["arm"] == arm]
            u = [r["decode_step_us"] for r in runs if r["arm"] == arm]
            summary[arm] = {"tok_s": v, "spread_pct": round(100 * (max(v) - min(v)) / min(v), 2),
                            "decode_step_us": u}
            summary[arm]["generate_ms_per_step"] = [r["generate_ms_per_step"] for r in runs if r["arm"] == arm]
            for key in ("decode_layer_us", "decode_layer_front_us", "decode_layer_hbm_peak_fraction",
                        "decode_mlp_us", "decode_mlp_hbm_peak_fraction"):
                w = [r[key] for r in runs if r["arm"] == arm and key in r]
                if w:
                    summary[arm][key] = w
        mean = lambda arm: sum(summary[arm]["tok_s"]) / len(summary[arm]["tok_s"])   # noqa: E731
        for a, b in (("fp8", "bf16"), ("fp8_block", "bf16"), ("fp8", "bf16_per_op"), ("fp8_mlp", "bf16"),
                     ("fp8_mlp", "fp8"), ("fp8_mlp", "fp8_block")):
            if a in arms and b in arms:
                summary[f"{a}_vs_{b}"] = round(mean(a) / mean(b), 4)
        f.write(json.dumps(summary) + "\n")
        print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    main()

"""Time the one-launch pass with non-default hyper-parameters (`PassParams`: channel ratio, softmax temperature,
Gaussian scales) against the default pass and against the route it replaces -- the stage-by-stage chain
(tests/_stage_chain.hook_chain over vidcom2_amd: select_low_var_channels -> compute_gaussian_scores -> compute_scales ->
select_outlier_indices -> _map_linear_offset, which materialises the selected columns and takes several launches and
host syncs).

Shape 128 x 196 x 3584 in bf16 and fp16, retain 0.25.  Settings: the default pass; ratio 0.25 / 0.75 / 1.0; temp 0.05;
alphas of 1, 3 (no powers of two) and 8 scales (2^-5 .. 2^2: half of them push exp's argument out of the v_exp_f32
window, into the fp64 exp).  Per setting and round, hipEvent medians of
    plan_us    CompressPlan.enqueue alone (the device time of the pass, no host sync inside the window)
    call_us    vidcom2_amd.compress(..., gather=False, params=...): the one-shot call with its single host sync
    stage_us   the stage chain at the same ratio / temp (alpha-only settings have no stage route: the stage functions
               take the reference's five scales) -- like call_us it ends with the kept indices known to the host
`--rounds` rounds alternate every setting's fused and stage legs; a record holds the median of the round medians, their
range, and whether the fused and stage ranges overlap.  One JSON line per (dtype, setting) on stdout and, with --out,
appended to that file (profiles/pass_params.jsonl).

    python scripts/pass_params.py [--rounds 5] [--iters 30] [--stage-iters 6] [--out profiles/pass_params.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import vidcom2_amd as vc  # noqa: E402
from vidcom2_amd import PassParams, synth  # noqa: E402
from vidcom2_amd.vidcom2 import CompressPlan  # noqa: E402

from _stage_chain import hook_chain  # noqa: E402

F, N, D, BASE = 128, 196, 3584, 0.25
A1, A3, A8 = [1.0], [0.1, 0.3, 3.0], [2.0 ** k for k in range(-5, 3)]
# name, ratio, temp, alphas (None: the reference's value)
SETTINGS = [("default", None, None, None), ("ratio0.25", 0.25, None, None), ("ratio0.75", 0.75, None, None),
            ("ratio1.0", 1.0, None, None), ("temp0.05", None, 0.05, None), ("alphas1", None, None, A1),
            ("alphas3", None, None, A3), ("alphas8", None, None, A8)]


def params_of(ratio, temp, alphas):
    kw = {}
    if ratio is not None:
        kw["channel_ratio"] = ratio
    if temp is not None:
        kw["temp"] = temp
    if alphas is not None:
        kw["alphas"] = alphas
    return PassParams(**kw) if kw else None


def timed(fn, iters, warmup):
    """Median microseconds of fn() between two device events (fn may synchronise inside: then the window is wall time)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def summary(vals):
    return {"median": round(statistics.median(vals), 1), "min": round(min(vals), 1), "max": round(max(vals), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--stage-iters", type=int, default=6)
    ap.add_argument("--dtypes", default="bf16,f16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/pass_params.py measures on the GPU: no ROCm device found")
    dev = torch.device("cuda")
    for dn in a.dtypes.split(","):
        dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dn]
        x = synth.make(F, N, D, dtype, seed=0, dist="drift").to(dev)
        legs = {}
        for name, ratio, temp, alphas in SETTINGS:
            P = params_of(ratio, temp, alphas)
            plan = CompressPlan(F, N, D, dtype, dev, BASE, gather=False, params=P)

            def run_plan(plan=plan):
                plan.enqueue(x)

            def run_call(P=P):
                vc.compress(x, N, BASE, gather=False, params=P)

            stage = None
            if alphas is None and P is not None:
                def stage(ratio=ratio, temp=temp):
                    hook_chain(vc, x, N, BASE, ratio, temp)
            # once, outside the timed windows: the fused pass and the stage route keep the same tokens
            got = vc.compress(x, N, BASE, gather=False, params=P)
            same = None if stage is None else bool(torch.equal(got.global_idx, hook_chain(vc, x, N, BASE, ratio, temp)["keep"]))
            legs[name] = dict(plan=run_plan, call=run_call, stage=stage, same=same, K=got.K,
                              times={"plan_us": [], "call_us": [], "stage_us": []})
        for rnd in range(a.rounds):                       # every round visits every setting: fused legs, then its stage leg
            for name, leg in legs.items():
                leg["times"]["plan_us"].append(timed(leg["plan"], a.iters, 5 if rnd == 0 else 2))
                leg["times"]["call_us"].append(timed(leg["call"], a.iters, 5 if rnd == 0 else 2))
                if leg["stage"] is not None:
                    leg["times"]["stage_us"].append(timed(leg["stage"], a.stage_iters, 2 if rnd == 0 else 1))
        base = statistics.median(legs["default"]["times"]["plan_us"])
        for name, ratio, temp, alphas in SETTINGS:
            leg = legs[name]
            rec = {"shape": [F, N, D], "dtype": dn, "base_scale": BASE, "setting": name, "channel_ratio": ratio, "temp": temp,
                   "alphas": alphas, "K": leg["K"], "rounds": a.rounds, "iters": a.iters}
            for k, vals in leg["times"].items():
                if vals:
                    rec[k] = summary(vals)
            rec["plan_vs_default"] = round(rec["plan_us"]["median"] / base, 3)
            if leg["stage"] is not None:
                rec["stage_iters"] = a.stage_iters
                rec["kept_indices_equal_stage_route"] = leg["same"]
                rec["ranges_overlap"] = not (rec["call_us"]["max"] < rec["stage_us"]["min"])
                rec["stage_over_call"] = round(rec["stage_us"]["median"] / rec["call_us"]["median"], 1)
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""Time the fp32-scored pass over 16-bit inputs (`score_dtype=torch.float32`) against the passes next to it.

Shape 128 x 196 x 3584 in bf16 and fp16, retain 0.25, `synth` inputs.  One process, the legs alternating inside every
round; per leg the device time of `CompressPlan.enqueue` between two hipEvents (no host sync inside the window):
    new           the fp32-scored pass on the 16-bit tensor
    native        the native 16-bit pass, default ("torch") mode
    native_exact  the native 16-bit pass, "exact" mode
    fp32_input    the fp32-input pass on the PRE-WIDENED tensor (the widening is not timed)
    widen_fp32    x.float() + the fp32-input pass: what a user does today for the fp32 decision
A round's figure is the median of `--iters` passes after `--warmup`; a leg's record holds the median of the round
medians and their range (the run-to-run spread).  The gate of the feature: `new` faster than `fp32_input` by more than
the spread of the two legs -- the ranges must not overlap.  The other two comparisons are reported, not gated.
Writes profiles/score_dtype_bench.json (one record per dtype).

    python scripts/score_dtype.py [--rounds 5] [--iters 30] [--warmup 10] [--out profiles/score_dtype_bench.json]
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

from vidcom2_amd import _ffi, synth  # noqa: E402
from vidcom2_amd.vidcom2 import CompressPlan  # noqa: E402

F, N, D, BASE = 128, 196, 3584, 0.25
LEGS = ("new", "native", "native_exact", "fp32_input", "widen_fp32")


def timed(fn, iters, warmup):
    """Median microseconds of fn() between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def summary(vals):
    return {"median_us": round(statistics.median(vals), 1), "min_us": round(min(vals), 1), "max_us": round(max(vals), 1),
            "rounds": [round(v, 1) for v in vals]}


def one_dtype(dtype, args):
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, dtype, 0, "drift").to(dev)
    x32 = x.float()
    _ffi.set_mode("torch")
    p_new = CompressPlan(F, N, D, dtype, dev, BASE, score_dtype=torch.float32)
    p_nat = CompressPlan(F, N, D, dtype, dev, BASE)
    p_32 = CompressPlan(F, N, D, torch.float32, dev, BASE)

    def exact():
        _ffi.set_mode("exact")
        try:
            p_nat.enqueue(x)
        finally:
            _ffi.set_mode("torch")

    legs = {"new": lambda: p_new.enqueue(x), "native": lambda: p_nat.enqueue(x), "native_exact": exact,
            "fp32_input": lambda: p_32.enqueue(x32), "widen_fp32": lambda: p_32.enqueue(x.float())}
    # the kept sets, once: the new pass and the fp32-input pass must agree before their times are compared
    p_new.enqueue(x)
    a = p_new.finish()
    p_32.enqueue(x32)
    b = p_32.finish()
    same = a.ks.tolist() == b.ks.tolist() and bool(torch.equal(a.global_idx, b.global_idx))
    p_nat.enqueue(x)
    c = p_nat.finish()
    kept = set(a.global_idx.tolist())
    overlap = len(kept & set(c.global_idx.tolist())) / max(1, len(kept))
    rounds = {k: [] for k in LEGS}
    for _ in range(args.rounds):
        for k in LEGS:
            rounds[k].append(timed(legs[k], args.iters, args.warmup))
    rec = {"dtype": str(dtype).replace("torch.", ""), "shape": [F, N, D], "base": BASE, "dist": "drift", "seed": 0,
           "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup,
           "new_equals_fp32_input_kept_set": same, "native_overlap_with_new": round(overlap, 4),
           "legs": {k: summary(v) for k, v in rounds.items()}}
    L = rec["legs"]
    rec["gate_new_faster_than_fp32_input_beyond_spread"] = L["new"]["max_us"] < L["fp32_input"]["min_us"]
    rec["new_minus_native_exact_us"] = round(L["new"]["median_us"] - L["native_exact"]["median_us"], 1)
    rec["saving_vs_widen_fp32_us"] = round(L["widen_fp32"]["median_us"] - L["new"]["median_us"], 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_dtype_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    out = {"script": "scripts/score_dtype.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "records": []}
    for dtype in (torch.bfloat16, torch.float16):
        rec = one_dtype(dtype, args)
        print(json.dumps(rec), flush=True)
        out["records"].append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

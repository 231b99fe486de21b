"""Time LLaVA-Video's grid pass with the newline stream (today's route) against the pass that never builds it
(`newline=`, k_gather_rows_grid).

Shape 64 x 169 x 3584 (LLaVA-Video-7B) in bf16 and fp16, retain 0.25, `synth` inputs.  One process, the legs alternating
inside every round; per leg the device time between two hipEvents (no host sync inside the window):
    today        the three stream-building copies upstream's add_token_per_grid and `_prep` make -- a torch restatement:
                 channel-major permute().contiguous(), torch.cat of the newline column, the transposed view made
                 contiguous -- followed by CompressPlan.enqueue(flat, img)
    new          CompressPlan.enqueue(flat, newline=vec)
    stream_only  the three copies on their own
    linear       the linear-mapper pass at the same shape (CompressPlan.enqueue(flat))
A round's figure is the median of `--iters` passes after `--warmup`; a leg's record holds the median of the round medians
and their range (the run-to-run spread).  The gather launch of each route (k_gather_rows / k_gather_rows_grid) comes from
vc2_profile_collect in a pass of its own at the end (per-kernel timing changes the launches in front of it).
Gates, applied to the output: `new` faster than `today` by more than the two legs' spread (the ranges do not overlap), and
`new` within the spread of `linear` (their ranges overlap).  Writes profiles/grid_newline_bench.json.

    python scripts/grid_newline_bench.py [--rounds 5] [--iters 30] [--warmup 10] [--out profiles/grid_newline_bench.json]
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

F, H, D, BASE = 64, 13, 3584, 0.25
N = H * H
LEGS = ("today", "new", "stream_only", "linear")


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


def build_stream(feat, nl):
    """The newline stream [F*h*(h+1), D] the way upstream builds it and `_prep` finishes it: three full-tensor copies."""
    cm = feat.view(F, H, H, D).permute(3, 0, 1, 2).contiguous()                          # 1: channel-major [D, F, h, h]
    cm = torch.cat((cm.view(D, F * H, H), nl[:, None, None].expand(D, F * H, 1)), dim=-1)   # 2: the newline column
    return cm.view(D, F * H * (H + 1)).t().contiguous()                                  # 3: the transposed view, copied


def gather_us(fn, n=20):
    """Mean microseconds per launch of the gather kernels over n passes, from vc2_profile_collect."""
    _ffi.profile_enable(True)
    try:
        _ffi.profile_collect()
        before = _ffi.profile_collect()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        after = _ffi.profile_collect()
    finally:
        _ffi.profile_enable(False)
    out = {}
    for k in ("k_gather_rows", "k_gather_rows_grid"):
        ms = after.get(k, (0.0, 0))[0] - before.get(k, (0.0, 0))[0]
        cnt = after.get(k, (0.0, 0))[1] - before.get(k, (0.0, 0))[1]
        if cnt:
            out[k] = {"us_per_launch": round(ms * 1e3 / cnt, 2), "launches": cnt}
    return out


def one_dtype(dtype, args):
    dev = torch.device("cuda:0")
    flat = synth.make(F, N, D, dtype, 0, "drift").to(dev)
    feat = flat.view(F, N, D)
    nl = torch.randn(D, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    _ffi.set_mode("torch")
    p_grid = CompressPlan(F, N, D, dtype, dev, BASE, "grid_vid", H)
    p_new = CompressPlan(F, N, D, dtype, dev, BASE, "grid_vid", H)
    p_lin = CompressPlan(F, N, D, dtype, dev, BASE)
    legs = {"today": lambda: p_grid.enqueue(flat, build_stream(feat, nl)), "new": lambda: p_new.enqueue(flat, newline=nl),
            "stream_only": lambda: build_stream(feat, nl), "linear": lambda: p_lin.enqueue(flat)}
    # the two routes must give the same bits before their times are compared
    p_grid.enqueue(flat, build_stream(feat, nl))
    a = p_grid.finish()
    p_new.enqueue(flat, newline=nl)
    b = p_new.finish()
    it = torch.int16
    same = a.K == b.K and bool(torch.equal(a.global_idx, b.global_idx)) and bool(torch.equal(a.rows.view(it), b.rows.view(it)))
    rounds = {k: [] for k in LEGS}
    for _ in range(args.rounds):
        for k in LEGS:
            rounds[k].append(timed(legs[k], args.iters, args.warmup))
    es = 2
    rec = {"dtype": str(dtype).replace("torch.", ""), "shape": [F, N, D], "base": BASE, "dist": "drift", "seed": 0,
           "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup, "K": int(a.K),
           "routes_bit_identical": same,
           "stream_copy_bytes": (2 * F * N * D + (F * N * D + F * H * (H + 1) * D) + 2 * F * H * (H + 1) * D) * es,
           "legs": {k: summary(v) for k, v in rounds.items()}}
    L = rec["legs"]
    rec["gate_new_faster_than_today_beyond_spread"] = L["new"]["max_us"] < L["today"]["min_us"]
    rec["gate_new_within_spread_of_linear"] = L["new"]["min_us"] <= L["linear"]["max_us"] and \
        L["linear"]["min_us"] <= L["new"]["max_us"]
    rec["saving_us"] = round(L["today"]["median_us"] - L["new"]["median_us"], 1)
    rec["new_minus_linear_us"] = round(L["new"]["median_us"] - L["linear"]["median_us"], 1)
    rec["gather_today"] = gather_us(legs["today"])
    rec["gather_new"] = gather_us(legs["new"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_newline_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    out = {"script": "scripts/grid_newline_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
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

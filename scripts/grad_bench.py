"""Time the backward of the kept-row gather (vc2_rows_grad) against torch's backward of `x[idx]` on the same indices.

Two legs: the target shape (128 x 196 x 3584 bf16, retain 0.25) and the cfg5 clip (128 x 196 x 4096 fp16).  Each leg
builds the forward graph once (`vidcom2_amd.compress(x).rows` and `x[global_idx]`) and then times
`torch.autograd.grad(out, x, g, retain_graph=True)` for both, alternating, with device events after a warm-up.  It
reports the median microseconds and the share of 8 TB/s over the algorithmic bytes (R*D + K*D) * element size -- every
input-gradient element written once, every kept-row gradient read once -- and checks once that both gradients have the
same bits.  One JSON line per leg on stdout.

    python scripts/grad_bench.py [--iters 50] [--warmup 10]
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/grad_bench.py --iters 10     (kernel times)
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import vidcom2_amd as vc  # noqa: E402

LEGS = {"target": (128, 196, 3584, torch.bfloat16), "cfg5": (128, 196, 4096, torch.float16)}
PEAK = 8e12


def leg(name, F, N, D, dtype, iters, warmup):
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(F * N, D, generator=gen, device=dev).to(dtype).requires_grad_()
    res = vc.compress(x, N, 0.25)                       # HIP forward with the backward attached
    idx = res.global_idx
    ref = x[idx]                                         # torch's forward on the same indices
    g = torch.randn(res.K, D, generator=gen, device=dev).to(dtype)
    hip = lambda: torch.autograd.grad(res.rows, x, g, retain_graph=True)[0]   # noqa: E731
    tch = lambda: torch.autograd.grad(ref, x, g, retain_graph=True)[0]        # noqa: E731
    same = torch.equal(hip().view(torch.int16), tch().view(torch.int16))
    for _ in range(warmup):
        hip(), tch()
    times = {"hip": [], "torch": []}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for i in range(iters):
        order = (("hip", hip), ("torch", tch)) if i % 2 == 0 else (("torch", tch), ("hip", hip))
        for k, (which, fn) in enumerate(order):
            ev[2 * k].record()
            fn()
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        for k, (which, _) in enumerate(order):
            times[which].append(ev[2 * k].elapsed_time(ev[2 * k + 1]) * 1e3)
    nbytes = (F * N * D + res.K * D) * x.element_size()
    out = {"leg": name, "shape": [F, N, D], "dtype": str(dtype).replace("torch.", ""), "K": res.K,
           "algorithmic_bytes": nbytes, "bits_equal": bool(same), "iters": iters}
    for which, ts in times.items():
        us = statistics.median(ts)
        out[f"{which}_us"] = round(us, 2)
        out[f"{which}_us_min"] = round(min(ts), 2)
        out[f"{which}_share_of_8TBps"] = round(nbytes / (us * 1e-6) / PEAK, 3)
    out["speedup"] = round(out["torch_us"] / out["hip_us"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--legs", default="target,cfg5")
    a = ap.parse_args()
    for name in a.legs.split(","):
        print(json.dumps(leg(name, *LEGS[name], a.iters, a.warmup)), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Batched prefill pruning step (Qwen-VL hooks, VC2_BATCHED_PREFILL=1) at B = 8, one video_grid_thw (32, 32, 32) bf16
video per row (32 frames x 256 tokens), D = 3584 (Qwen2.5-VL-7B), left-padded prompts of different text lengths.
Prints one JSON line:

  batched_ms     hipEvent time of the batched step: scoring of the 8 videos (compress_batch lanes, one host sync for the
                 counts) + vc2_keep_positions_batched + vc2_repad_rows
  sequential_ms  the same prompts pruned as 8 batch-1 hook steps (_compute_keep_indices + keep_positions +
                 gather_scatter per row)
  repad_bytes    algorithmic bytes of the re-pad gather (kept rows read + every row of [B, S', D] written)

With --kstats <rocprofv3 kernel_stats.csv> (a separate `rocprofv3 --kernel-trace --stats -- python <this> --repad-only`
run) also the re-pad kernel's average time and its bytes / time as a fraction of 8 TB/s.

    python scripts/batched_prefill.py [--steps 20] [--warmup 5] [--repad-only] [--kstats FILE]
"""
import argparse
import csv
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vidcom2_amd import synth                                        # noqa: E402
from vidcom2_amd.fused import gather_scatter, keep_positions, keep_positions_batched, repad_rows   # noqa: E402
from vidcom2_amd.models.qwen2_5_vl import _compute_keep_indices, _compute_keep_indices_many   # noqa: E402

B, D, GRID, MERGE, R = 8, 3584, (32, 32, 32), 2, 0.25
N_VID = GRID[0] * GRID[1] * GRID[2] // MERGE ** 2


def inputs(dev):
    lens = [40 + 23 * b for b in range(B)]                           # text tokens per prompt
    S = N_VID + max(lens)
    vm = torch.zeros((B, S), dtype=torch.bool)
    am = torch.zeros((B, S), dtype=torch.int64)
    for b, n in enumerate(lens):
        L = N_VID + n
        am[b, S - L:] = 1
        vm[b, S - L + n // 2: S - L + n // 2 + N_VID] = True
    embeds = synth.make(B, S, D, torch.bfloat16, seed=5, dist="iid").reshape(B, S, D).to(dev)
    feats = [embeds[b][vm[b].to(dev)].contiguous() for b in range(B)]
    return embeds, vm.to(dev), am.to(dev), feats


def batched_step(embeds, vm, am, feats, grids):
    kept = _compute_keep_indices_many(feats, grids, MERGE, R)
    lay = keep_positions_batched(vm, kept, B * N_VID, True, None, am)
    return repad_rows(embeds, lay.keep)


def sequential_step(embeds, vm, am, feats, grids):
    out = []
    for b in range(B):                                               # (each row alone, its padding removed)
        n_pad = embeds.shape[1] - N_VID - (40 + 23 * b)
        row_vm = vm[b, n_pad:]
        kept = _compute_keep_indices(feats[b], grids[b], MERGE, R)
        keep, _ = keep_positions(row_vm, kept, N_VID)
        out.append(gather_scatter([embeds[b, n_pad:]], keep, check=False)[0])
    return out


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def repad_kernel_ns(path):
    for r in csv.DictReader(open(path)):
        if "k_repad_rows" in r["Name"]:
            return float(r["AverageNs"])
    raise SystemExit(f"no k_repad_rows row in {path}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repad-only", action="store_true", help="only the re-pad launch, steps times (for rocprofv3)")
    ap.add_argument("--kstats", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    embeds, vm, am, feats = inputs(dev)
    grids = torch.tensor([GRID] * B)
    kept = _compute_keep_indices_many(feats, grids, MERGE, R)
    lay = keep_positions_batched(vm, kept, B * N_VID, True, None, am)
    n_kept_rows = int(lay.lengths.sum()) - int((am == 0).sum())      # rows of the prompts' own content
    repad_bytes = (int(lay.lengths.sum()) + B * lay.S) * D * 2         # kept rows read, every slot written
    res = dict(metric="batched_prefill_prune", B=B, S=int(embeds.shape[1]), S_pruned=lay.S, D=D, dtype="bf16",
               grid=list(GRID), kept_rows=n_kept_rows, repad_bytes=repad_bytes)
    if a.repad_only:
        for _ in range(a.steps):
            repad_rows(embeds, lay.keep)
        torch.cuda.synchronize()
    else:
        res["batched_ms"] = timed(lambda: batched_step(embeds, vm, am, feats, grids), a.steps, a.warmup)
        res["sequential_ms"] = timed(lambda: sequential_step(embeds, vm, am, feats, grids), a.steps, a.warmup)
        res["repad_ms_event"] = timed(lambda: repad_rows(embeds, lay.keep), a.steps, a.warmup)
    if a.kstats:
        ns = repad_kernel_ns(a.kstats)
        res["repad_kernel_us"] = ns / 1e3
        res["repad_frac_of_8TBps"] = repad_bytes / (ns * 1e-9) / 8e12
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

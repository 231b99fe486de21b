"""Time one logical rank's stage chain of the frame-sharded pass (chan_stats -> select_channels -> phase1 -> vc_blocks ->
phase2 -> select) for equal and unequal layouts of a 512-frame bf16 clip at 196 x 3584 over 8 ranks:

    equal        8 x 64 frames
    off_by_one   (64, 64, 64, 64, 64, 64, 65, 63)
    fps500       shard_frames(500, 8) of the clip's first 500 frames

All ranks run once outside the timed window; what the all-gathers would deliver (stat blocks, group sums, replay
records, s) is kept on the device.  The timed window is ONE rank's chain on those inputs: the five stage calls and, with
an unequal layout, that rank's padding copies and the compactions of the padded exchanges (no collective: multi-process
RCCL is measured by the benchmark's multi-GPU run).  `torch` mode.  `--rounds` rounds alternate the legs; a record holds
the median of the round medians (hipEvents) and their range.

The `equal` leg uses only what HipStages has always offered -- HipStages(F, N, D, dtype, device, base), F_total set
afterwards, the stage calls on stacked exchanges -- so this file also runs in a tree without the unequal layouts (the
other legs are skipped there): run it in both trees in one sitting to compare the equal leg.

    python scripts/ragged_shards.py [--rounds 5] [--iters 20] [--label this] [--out profiles/ragged_shards.jsonl]
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vidcom2_amd import sharded, synth  # noqa: E402
from vidcom2_amd.sharded import HipStages  # noqa: E402

N, D, BASE, WORLD, F_CLIP = 196, 3584, 0.25, 8, 512
HAS_LAYOUTS = "frames" in inspect.signature(HipStages.__init__).parameters


class Leg:
    """One layout: every rank's stages, the exchanged tensors of one full pass, and the timed rank's chain."""

    def __init__(self, name, frames, x, dev, timed_rank):
        self.name, self.frames, self.rank = name, list(frames), timed_rank
        self.F, self.ragged = sum(frames), len(set(frames)) > 1
        self.f0s = [sum(frames[:p]) for p in range(len(frames))]
        self.shards = [x[f0 * N: (f0 + f) * N] for f0, f in zip(self.f0s, frames)]
        if self.ragged:
            self.st = [HipStages(f, N, D, torch.bfloat16, dev, BASE, frames=self.frames, rank=p)
                       for p, f in enumerate(frames)]
        else:
            self.st = [HipStages(f, N, D, torch.bfloat16, dev, BASE) for f in frames]
        for s in self.st:
            s.F_total = self.F
        self.R = self.F * N
        self._prepare()

    def _exchange(self, parts, counts):
        """What the all-gather of `parts` delivers: the stack ([world, ...]; padded with an unequal layout)."""
        if not self.ragged:
            return torch.stack([t.clone() for t in parts])
        return torch.stack([sharded.pad_rows(t, max(counts)).clone() for t in parts])

    def _consume(self, gathered, idx, out):
        return sharded.compact_rows(gathered, idx, out) if self.ragged else gathered

    def _prepare(self):
        st, sh, R = self.st, self.shards, self.R
        bf = st[0].bf
        self.nb = [f // bf for f in self.frames]
        dev = sh[0].device
        if self.ragged:
            self.i_stats, self.i_s = sharded.compact_index(self.nb, dev), sharded.compact_index(self.frames, dev)
            self.o_stats = torch.empty((sum(self.nb), 2, D), dtype=torch.float64, device=dev)
            self.o_s = torch.empty(self.F, dtype=torch.float32, device=dev)
            self.p_stats = torch.zeros((max(self.nb), 2, D), dtype=torch.float64, device=dev)
            self.p_s = torch.zeros(max(self.frames), dtype=torch.float32, device=dev)
        else:
            self.i_stats = self.i_s = self.o_stats = self.o_s = None
        self.g_stats = self._exchange([s.chan_stats(xs) for s, xs in zip(st, sh)], self.nb)
        stats_all = self._consume(self.g_stats, self.i_stats, self.o_stats)
        for s in st:
            s.select_channels(stats_all, R)
        self.g_csum = torch.stack([s.phase1(xs).clone() for s, xs in zip(st, sh)])
        blocks = [s.vc_blocks(xs, self.g_csum, R, f0) for s, xs, f0 in zip(st, sh, self.f0s)]
        assert all(b is not None for b in blocks), "the replay applies to this shape in torch mode"
        self.g_blocks = torch.stack([b.clone() for b in blocks])
        self.g_s = self._exchange([s.phase2(xs, self.g_csum, R, self.g_blocks) for s, xs in zip(st, sh)], self.frames)
        s_all = self._consume(self.g_s, self.i_s, self.o_s).reshape(-1)
        self.K = 0
        for s, xs, f0 in zip(st, sh, self.f0s):
            s.select(xs, s_all, f0)
            self.K += s.result(f0).K
        torch.cuda.synchronize()

    def run(self):
        """The timed rank's chain; its own messages are padded like ShardedCompressor pads them, the gathered inputs are
        the prepared ones."""
        s, x, R, f0 = self.st[self.rank], self.shards[self.rank], self.R, self.f0s[self.rank]
        stats = s.chan_stats(x)
        if self.ragged:
            sharded.pad_rows(stats, self.p_stats.shape[0], self.p_stats)
        s.select_channels(self._consume(self.g_stats, self.i_stats, self.o_stats), R)
        s.phase1(x)
        s.vc_blocks(x, self.g_csum, R, f0)
        s_loc = s.phase2(x, self.g_csum, R, self.g_blocks)
        if self.ragged:
            sharded.pad_rows(s_loc, self.p_s.shape[0], self.p_s)
        s.select(x, self._consume(self.g_s, self.i_s, self.o_s).reshape(-1), f0)


def timed(fn, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--label", default="this", help="which tree this run measures (recorded in every line)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/ragged_shards.py measures on the GPU: no ROCm device found")
    dev = torch.device("cuda")
    x = synth.make(F_CLIP, N, D, torch.bfloat16, seed=0, dist="drift").to(dev)
    # rank 0 holds 64 frames in every layout: the same sweeps; in `off_by_one` it pads all three of its messages
    layouts = [("equal", [F_CLIP // WORLD] * WORLD, 0)]
    if HAS_LAYOUTS:
        layouts += [("off_by_one", [64, 64, 64, 64, 64, 64, 65, 63], 0), ("fps500", sharded.shard_frames(500, WORLD), 0)]
    legs = [Leg(name, frames, x, dev, r) for name, frames, r in layouts]
    times = {leg.name: [] for leg in legs}
    for rnd in range(max(5, a.rounds)):                                # the legs alternate within every round
        for leg in legs:
            times[leg.name].append(timed(leg.run, a.iters, 5 if rnd == 0 else 2))
    base = statistics.median(times["equal"])
    for leg in legs:
        v = times[leg.name]
        rec = {"label": a.label, "layout": leg.name, "frames": leg.frames, "timed_rank": leg.rank,
               "timed_rank_frames": leg.frames[leg.rank], "shape": [leg.F, N, D], "dtype": "bf16", "mode": "torch",
               "stat_block_frames": leg.st[0].bf, "K": leg.K, "rounds": len(v), "iters": a.iters,
               "chain_us": {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)},
               "vs_equal": round(statistics.median(v) / base, 3)}
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()

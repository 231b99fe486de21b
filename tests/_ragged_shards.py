"""Unequal frame counts per rank in the frame-sharded pass -- TEST ONLY helpers.

RaggedOracleStages   the oracle-backed CPU stages of _oracle_stages.py, taking the layout ShardedCompressor hands over
emulate_ragged_ranks logical ranks with a list of frame counts on ONE device through the HIP stage entry points, the
                     exchanges done by padding + stacking + compacting (what the padded all-gather returns)
gloo_worker          one rank of a gloo process group on the CPU (spawned by tests/test_ragged_shards.py)
gpu_gloo_child       one rank of a two-process group sharing cuda:0 (its own process: `python _ragged_shards.py ...`)
"""
import os
import sys

import torch
import torch.distributed as dist

import oracle as O
from vidcom2_amd import synth
from vidcom2_amd.sharded import (HipStages, ShardedCompressor, compact_index, compact_rows, pad_rows,
                                 stat_block_frames)

from _oracle_stages import OracleStages

DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}


class RaggedOracleStages(OracleStages):
    """With unequal shards chan_stats returns one (mean, M2) per stat block of `bf` frames ([F_p / bf, 2, D]: the rows
    ShardedCompressor pads and compacts), and select_channels folds the gathered blocks weighted by their row counts."""

    def set_layout(self, frames, rank):
        assert frames[rank] == self.F
        self.frames, self.rank = list(frames), rank
        self.bf = stat_block_frames(frames)

    def chan_stats(self, x):
        xd = x.double().view(self.F // self.bf, self.bf * self.N, self.D)
        mean = xd.mean(1)
        return torch.stack([mean, ((xd - mean[:, None]) ** 2).sum(1)], dim=1)

    def select_channels(self, stats_all, R_total):
        nb = sum(f // self.bf for f in self.frames)
        assert tuple(stats_all.shape) == (nb, 2, self.D)
        n = torch.full((nb, 1), float(self.bf * self.N), dtype=torch.float64)      # rows behind every (mean, M2)
        assert int(n.sum()) == R_total
        mean = (n * stats_all[:, 0]).sum(0) / R_total
        m2 = (stats_all[:, 1] + n * (stats_all[:, 0] - mean) ** 2).sum(0)
        var = (m2 / R_total).float().to(self.dtype)
        self.chan_idx = O.topk_smallest(var, int(self.D * 0.5), True)


def gloo_worker(rank, frames, shape, dtype_name, dist_name, seed, port, q):
    world = len(frames)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, base = shape
        dtype = DTYPES[dtype_name]
        x = synth.make(F, N, D, dtype, seed, dist_name)
        f0, Fl = sum(frames[:rank]), frames[rank]
        xl = x[f0 * N: (f0 + Fl) * N].contiguous()
        sc = ShardedCompressor(Fl, N, D, dtype, "cpu", base, stages=RaggedOracleStages(Fl, N, D, dtype, base))
        assert sc.frames == list(frames) and sc.f0 == f0 and sc.F_total == F
        res = sc(xl)
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert counts[rank] == res.K and torch.equal(rows_all, x[gidx_all])
        q.put((rank, res.global_idx.tolist(), res.ks.tolist(), gidx_all.tolist()))
    finally:
        dist.destroy_process_group()


def emulate_ragged_ranks(x, frames, N, D, dtype, base, dev, vc_cap=64, spy=None):
    """len(frames) logical ranks, one HipStages each (built with the layout), the exchanges as the padded all-gather
    + compaction of ShardedCompressor would deliver them.  spy(stages) may wrap a rank's library handle.
    Returns (results, stages, exchanged) -- `exchanged` holds the gathered stat blocks."""
    W, F = len(frames), sum(frames)
    f0s = [sum(frames[:p]) for p in range(W)]
    shards = [x[f0 * N: (f0 + f) * N].contiguous() for f0, f in zip(f0s, frames)]
    st = [HipStages(f, N, D, dtype, dev, base, vc_cap=vc_cap, frames=frames, rank=p) for p, f in enumerate(frames)]
    for s in st:
        s.F_total = F
        if spy is not None:
            spy(s)
    ragged = len(set(frames)) > 1

    def exchange(parts, counts):
        if not ragged:
            return torch.stack([t.clone() for t in parts])
        got = torch.stack([pad_rows(t, max(counts)).clone() for t in parts])
        return compact_rows(got, compact_index(counts, got.device))

    bf = st[0].bf
    assert all(s.bf == bf for s in st)
    stats_all = exchange([s.chan_stats(xs) for s, xs in zip(st, shards)], [f // bf for f in frames])
    for s in st:
        s.select_channels(stats_all, F * N)
    csum_all = torch.stack([s.phase1(xs).clone() for s, xs in zip(st, shards)])
    blocks = [s.vc_blocks(xs, csum_all, F * N, f0) for s, xs, f0 in zip(st, shards, f0s)]
    assert len({b is None for b in blocks}) == 1
    if blocks[0] is not None and st[0].needs_rounds():
        counts = [s.flagged_columns() for s in st]
        assert len(set(counts)) == 1, counts
        for j0 in range(0, max(counts[0], 1), st[0].vc_cap):
            if j0:
                blocks = [s.vc_blocks_round(xs, F * N, f0, j0) for s, xs, f0 in zip(st, shards, f0s)]
            blocks_all = torch.stack([b.clone() for b in blocks])
            for s in st:
                s.vc_finish_round(F * N, blocks_all, j0)
        s_parts = [s.phase2(xs, csum_all, F * N, vc_final=True).clone() for s, xs in zip(st, shards)]
    elif blocks[0] is not None:
        blocks_all = torch.stack([b.clone() for b in blocks])
        s_parts = [s.phase2(xs, csum_all, F * N, blocks_all).clone() for s, xs in zip(st, shards)]
    else:
        s_parts = [s.phase2(xs, csum_all, F * N).clone() for s, xs in zip(st, shards)]
    s_all = exchange(s_parts, list(frames)).reshape(-1)
    out = []
    for s, xs, f0 in zip(st, shards, f0s):
        s.select(xs, s_all, f0)
        out.append(s.result(f0))
    return out, st, {"stats": stats_all}


def gpu_gloo_child(rank, frames, port, out_path):
    """One rank of a gloo group whose ranks share cuda:0: the real HIP stages behind ShardedCompressor and a real
    collective, unequal shards of synth.make(8, 49, 64, bf16, 2, "drift")."""
    world = len(frames)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, base = sum(frames), 49, 64, 0.25
        dev = torch.device("cuda:0")
        x = synth.make(F, N, D, torch.bfloat16, 2, "drift")
        f0, Fl = sum(frames[:rank]), frames[rank]
        sc = ShardedCompressor(Fl, N, D, torch.bfloat16, dev, base)
        assert sc.ragged and sc.stages.ragged and sc.f0 == f0
        res = sc(x[f0 * N: (f0 + Fl) * N].contiguous().to(dev))
        torch.cuda.synchronize()
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert sum(counts) == rows_all.shape[0] and torch.equal(rows_all.cpu(), x[gidx_all.cpu()])
        torch.save({"gidx": res.global_idx.cpu(), "ks": res.ks.cpu(), "rows": res.rows.cpu(), "all": gidx_all.cpu()},
                   out_path)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    gpu_gloo_child(int(sys.argv[1]), [int(f) for f in sys.argv[2].split(",")], int(sys.argv[3]), sys.argv[4])

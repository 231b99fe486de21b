"""Pass parameters and the C % 32 tail replay in the frame-sharded pass -- TEST ONLY helpers.

emulate_ranks        logical ranks on ONE device through the HIP stage entry points, with params / score_dtype; the
                     exchanges by padding + stacking + compacting (what the padded all-gather returns)
ParamOracleStages    CPU stages that honour a PassParams, from the oracle's public functions
gloo_worker          one rank of a gloo group on the CPU (spawned by tests/test_sharded_params.py)
ctor_worker          one rank that only constructs a ShardedCompressor (params / score_dtype agreement)
gpu_gloo_child       one rank of a two-process group sharing cuda:0 (its own process: `python _sharded_params.py ...`)
four_chain_sum       row_sum's four interleaved chains over a list of fp32 values, restated in plain Python
tail_record_plan     the format of a tail column's exchange-2b record per rank (head / run / tail counts), restated
tail_records / tail_finish   the exchange-2b record of a tail column per rank, and the finisher over the gathered records
"""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

import oracle as O
from vidcom2_amd import PassParams, synth
from vidcom2_amd.sharded import HipStages, ShardedCompressor, compact_index, compact_rows, pad_rows
from vidcom2_amd.vidcom2 import cascade_level_power

from _ragged_shards import DTYPES, RaggedOracleStages

REF_ALPHAS = [2 ** k for k in range(-3, 2)]
GLOO_PARAMS = PassParams(0.25, 0.05, [0.1, 0.3, 1.0, 3.0])          # the fixture case `llava_vid` (linear keep indices)


def params_of(c):
    return PassParams(0.5 if c["ratio"] is None else c["ratio"], 0.01 if c["temp"] is None else c["temp"],
                      REF_ALPHAS if c.get("alphas") is None else c["alphas"])


def emulate_ranks(x, frames, N, D, dtype, base, dev, params=None, score_dtype=None, vc_cap=64, spy=None):
    """len(frames) logical ranks, one HipStages each.  Equal counts go through the equal-rank forms (no layout is handed
    over), unequal ones through the ragged forms.  Returns (results, stages)."""
    W, F = len(frames), sum(frames)
    ragged = len(set(frames)) > 1
    f0s = [sum(frames[:p]) for p in range(W)]
    shards = [x[f0 * N: (f0 + f) * N].contiguous() for f0, f in zip(f0s, frames)]
    st = [HipStages(f, N, D, dtype, dev, base, vc_cap=vc_cap, params=params, score_dtype=score_dtype,
                    **(dict(frames=frames, rank=p) if ragged else {})) for p, f in enumerate(frames)]
    for s in st:
        s.F_total = F
        if spy is not None:
            spy(s)

    def exchange(parts, counts):
        if not ragged:
            return torch.stack([t.clone() for t in parts])
        got = torch.stack([pad_rows(t, max(counts)).clone() for t in parts])
        return compact_rows(got, compact_index(counts, got.device))

    bf = st[0].bf
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
    return out, st


class ParamOracleStages(RaggedOracleStages):
    """The oracle-backed CPU stages with a PassParams: int(D * ratio) channels, the Gaussian scales in list order, the
    softmax temperature.  The rows are normalised by torch itself (the reference's own F.normalize on the CPU); the video
    centre is the exactly rounded mean of the all-gathered fp64 sums."""

    def __init__(self, F, N, D, dtype, base, params):
        super().__init__(F, N, D, dtype, base)
        self.params = params

    def select_channels(self, stats_all, R_total):
        super().select_channels(stats_all, R_total)
        nb = stats_all.shape[0]
        n = torch.full((nb, 1), float(self.bf * self.N), dtype=torch.float64)
        mean = (n * stats_all[:, 0]).sum(0) / R_total
        m2 = (stats_all[:, 1] + n * (stats_all[:, 0] - mean) ** 2).sum(0)
        var = (m2 / R_total).float().to(self.dtype)
        self.chan_idx = O.topk_smallest(var, self.params.channels(self.D), True)

    def _xhat(self, x):
        return torch.nn.functional.normalize(x[:, self.chan_idx], dim=-1).view(self.F, self.N, -1)

    def phase1(self, x):
        return self._xhat(x).double().sum((0, 1))

    def phase2(self, x, csum_all, R_total):
        xh = self._xhat(x)
        centre = (csum_all.reshape(-1, csum_all.shape[-1]).sum(0) / R_total).float().to(self.dtype)
        v = O.multi_scale_gaussian(xh, centre.view(1, 1, -1), list(self.params.alphas))
        f = O.multi_scale_gaussian(xh, xh.mean(1, keepdim=True), list(self.params.alphas))
        s, self.total = O.fuse(v, f)
        return s.float()

    def select(self, x, s_all, f0):
        scales = O.compute_scales(s_all.to(self.dtype), self.base, self.params.temp)[f0: f0 + self.F].contiguous()
        idx = O.select_outlier_indices(self.total, scales, self.N)
        self.ks = torch.tensor([i.numel() for i in idx], dtype=torch.int64)
        self.local = O.map_linear_offset(idx, self.N)
        self.rows = x[self.local]


def gloo_worker(rank, frames, case, port, q):
    world = len(frames)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, dn, seed, dname, base = case
        dtype = DTYPES[dn]
        x = synth.make(F, N, D, dtype, seed, dname)
        f0, Fl = sum(frames[:rank]), frames[rank]
        O.set_mode("torch")
        sc = ShardedCompressor(Fl, N, D, dtype, "cpu", base, params=GLOO_PARAMS,
                               stages=ParamOracleStages(Fl, N, D, dtype, base, GLOO_PARAMS))
        res = sc(x[f0 * N: (f0 + Fl) * N].contiguous())
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert counts[rank] == res.K and torch.equal(rows_all, x[gidx_all])
        q.put((rank, res.ks.tolist(), gidx_all.tolist()))
    finally:
        dist.destroy_process_group()


def ctor_worker(rank, world, port, kind, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        N, D, dtype, F = 49, 64, torch.bfloat16, 2 + rank
        params = {"params": PassParams(0.25 + 0.25 * rank), "temp": PassParams(temp=0.01 * (1 + rank)),
                  "alphas": PassParams(alphas=[1.0] * (1 + rank)), "none-vs-set": PassParams(0.25) if rank else None,
                  "equal": PassParams(0.25, 0.05, [1.0]), "default-vs-none": PassParams() if rank else None}.get(kind)
        sd = {"score_dtype": (None, torch.float32)[rank], "score-equal": torch.float32,
              "score-plain": (None, torch.bfloat16)[rank]}.get(kind)
        stages = RaggedOracleStages(F, N, D, dtype, 0.25)
        try:
            ShardedCompressor(F, N, D, dtype, "cpu", 0.25, stages=stages, params=params, score_dtype=sd)
            q.put((rank, "accepted", ""))
        except Exception as e:                                          # noqa: BLE001 (the parent judges the type)
            q.put((rank, type(e).__name__, str(e)))
    finally:
        dist.destroy_process_group()


GPU_CHILD_PARAMS = PassParams(0.75, 0.05, [0.1, 0.3, 1.0, 3.0])


def gpu_gloo_child(rank, frames, port, out_path):
    """One rank of a gloo group whose ranks share cuda:0: ShardedCompressor with params, the HIP stages, a real (padded)
    collective; unequal shards of synth.make(8, 49, 64, bf16, 2, "drift")."""
    world = len(frames)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, base = sum(frames), 49, 64, 0.25
        dev = torch.device("cuda:0")
        x = synth.make(F, N, D, torch.bfloat16, 2, "drift")
        f0, Fl = sum(frames[:rank]), frames[rank]
        sc = ShardedCompressor(Fl, N, D, torch.bfloat16, dev, base, params=GPU_CHILD_PARAMS)
        assert sc.ragged and sc.stages.ragged and sc.stages.C == 48 and sc.stages._opts is not None
        res = sc(x[f0 * N: (f0 + Fl) * N].contiguous().to(dev))
        torch.cuda.synchronize()
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert sum(counts) == rows_all.shape[0] and torch.equal(rows_all.cpu(), x[gidx_all.cpu()])
        torch.save({"gidx": res.global_idx.cpu(), "ks": res.ks.cpu(), "rows": res.rows.cpu(), "all": gidx_all.cpu(),
                    "fragile": sc.stages.vc_fragile}, out_path)
    finally:
        dist.destroy_process_group()


# ---- the four-chain order, restated ---------------------------------------------------------------------------------
f32 = np.float32


def _seq(vals):
    a = f32(vals[0])
    for v in vals[1:]:
        a = f32(a + f32(v))
    return a


def cascade_final(blocks, tail, lp):
    """torch's SumKernel cascade from the level-0 block sums and the < 2^lp leftover values: level-1 groups of B blocks,
    level-2 groups of B level-1 groups, then ((tail + acc1) + acc2) + acc3."""
    B = 1 << lp
    l1 = [_seq(blocks[g: g + B]) for g in range(0, len(blocks), B)]
    n1c = len(blocks) >> lp
    n2 = n1c >> lp
    acc3 = f32(0)
    for h in range(n2):
        acc3 = f32(acc3 + _seq(l1[B * h: B * h + B]))
    acc2 = f32(0)
    for g in range(B * n2, n1c):
        acc2 = f32(acc2 + l1[g])
    acc1 = l1[n1c] if len(blocks) & (B - 1) else f32(0)
    r = f32(0)
    for v in tail:
        r = f32(r + f32(v))
    return f32(f32(f32(r + acc1) + acc2) + acc3)


def four_chain_sum(vals):
    """row_sum over R values: chain k = the cascade over vals[k::4][:R // 4] with its own level power; chain 0, + the R % 4
    leftover values one by one, + chains 1, 2, 3."""
    R = len(vals)
    q4 = R >> 2
    lp4 = cascade_level_power(q4)
    B4 = 1 << lp4
    part = []
    for k in range(4):
        ch = [vals[k + 4 * e] for e in range(q4)]
        nb = q4 >> lp4
        part.append(cascade_final([_seq(ch[b * B4: (b + 1) * B4]) for b in range(nb)], ch[nb * B4:], lp4))
    s = part[0]
    for v in vals[q4 * 4:]:
        s = f32(s + f32(v))
    for k in (1, 2, 3):
        s = f32(s + part[k])
    return s


def tail_record_plan(frames_rows, R_total=None):
    """The format of a tail column's exchange-2b record (include/vc2.h, vc2_shard_opts.tail_records), restated; per rank
    (row0, head, runs, tail) -- `head` raw rows that end a run begun before the rank, `runs` aligned runs of 4 * B4 video
    rows it holds completely (four chain sums each), `tail` raw rows behind them -- and the run length.  frames_rows: every
    rank's row count in rank order."""
    R = sum(frames_rows) if R_total is None else int(R_total)
    run = 4 << cascade_level_power(R >> 2)
    out, row0 = [], 0
    for rows in frames_rows:
        head = min(rows, (run - row0 % run) % run)
        runs = (rows - head) // run
        out.append((row0, head, runs, rows - head - runs * run))
        row0 += rows
    return out, run


def tail_records(vals, rank_rows):
    """What every rank puts into the record of a tail column (tail_record_plan lays it out): (head raw values,
    tail raw values, four sums per complete run)."""
    plan, run = tail_record_plan(rank_rows)
    recs = []
    for row0, head, runs, tail in plan:
        mine = vals[row0: row0 + head + runs * run + tail]
        sums = [_seq(mine[head + i * run + k: head + (i + 1) * run: 4]) for i in range(runs) for k in range(4)]
        recs.append((list(mine[:head]), list(mine[head + runs * run:]), sums))
    return recs, plan, run


def tail_finish(recs, plan, run, R):
    """The finisher's order over the gathered records: complete runs from their owner's sums, a straddling run's rows one
    by one from whichever ranks hold them, then the four-chain combination."""
    starts = [p[0] for p in plan]

    def owner(r):
        return max(w for w, s0 in enumerate(starts) if s0 <= r)

    def row_value(r):
        w = owner(r)
        row0, head, runs, _ = plan[w]
        off = r - row0
        return recs[w][0][off] if off < head else recs[w][1][off - head - runs * run]

    def block_value(b, k):
        g0 = b * run
        w = owner(g0)
        row0, head, runs, _ = plan[w]
        off = g0 - row0
        if off >= head and (off - head) % run == 0 and (off - head) // run < runs:
            return recs[w][2][4 * ((off - head) // run) + k]
        return _seq([row_value(g0 + k + 4 * u) for u in range(run // 4)])

    q4 = R >> 2
    lp4 = cascade_level_power(q4)
    nb4 = q4 >> lp4
    part = [cascade_final([block_value(b, k) for b in range(nb4)],
                          [row_value(nb4 * run + k + 4 * e) for e in range(q4 - (nb4 << lp4))], lp4) for k in range(4)]
    s = part[0]
    for r in range(q4 * 4, R):
        s = f32(s + f32(row_value(r)))
    for k in (1, 2, 3):
        s = f32(s + part[k])
    return s


if __name__ == "__main__":
    gpu_gloo_child(int(sys.argv[1]), [int(f) for f in sys.argv[2].split(",")], int(sys.argv[3]), sys.argv[4])

"""Frame-sharded pass with UNEQUAL frame counts per rank.  CPU: gloo runs of the collective logic (padded all-gathers,
device-side compaction) with oracle-backed stages, and the host logic.  GPU: logical ranks on one device through the HIP
stage entry points -- the ragged forms of exchange 2b included -- against the unsharded pass and the oracle."""
import os
import socket
import subprocess
import sys
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle as O
from vidcom2_amd import synth
from vidcom2_amd.sharded import ShardedCompressor, shard_frames, stat_block_frames

from _oracle_stages import OracleStages
from _ragged_shards import DTYPES, RaggedOracleStages, emulate_ragged_ranks, gloo_worker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_SYMBOLS = ("vc2_video_centre_blocks_ragged", "vc2_video_centre_blocks_round_ragged",
                  "vc2_video_centre_finish_round_ragged", "vc2_scores_phase2_blocks_ragged")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# ---- CPU -----------------------------------------------------------------------------------------------------------

def _run_gloo(frames, shape, dtype_name, dist_name, seed):
    world = len(frames)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=gloo_worker, args=(r, list(frames), shape, dtype_name, dist_name, seed, port, q))
             for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = []
        while len(got) < world:
            try:
                got.append(q.get(timeout=1))
            except Exception:                                          # (queue.Empty)
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a rank ended with exit code {dead} (parent commit: the constructor's ValueError)"
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return sorted(got)


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_gloo_world3_unequal_shards_match_the_oracle(dtype_name):
    """8 x 49 x 64 split (3, 2, 3): budgets and kept indices of the concatenated ranks are the whole-pass oracle's, and
    gather_kept returns x[gidx] on every rank (asserted in the worker)."""
    shape, frames = (8, 49, 64, 0.25), (3, 2, 3)
    got = _run_gloo(frames, shape, dtype_name, "drift", 3)
    F, N, D, base = shape
    x = synth.make(F, N, D, DTYPES[dtype_name], 3, "drift")
    ref = O.compress_indices(x, N, base)
    assert sum((g[2] for g in got), []) == ref["ks"].tolist()
    assert sum((g[1] for g in got), []) == ref["global_idx"].tolist()
    for g in got:                                                       # every rank gathered all kept rows
        assert g[3] == ref["global_idx"].tolist()


def _emulate_cpu(x, frames, N, D, dtype, base):
    """The collective logic without processes: ShardedCompressor objects (world patched in) whose _gather is fed by
    running the ranks in lock step, stage by stage."""
    W, F = len(frames), sum(frames)
    f0s = [sum(frames[:p]) for p in range(W)]
    shards = [x[f0 * N: (f0 + f) * N].contiguous() for f0, f in zip(f0s, frames)]
    scs = []
    for p, f in enumerate(frames):
        sc = ShardedCompressor.__new__(ShardedCompressor)
        sc.group, sc.always_collective, sc._xev, sc.world, sc.rank = None, False, None, W, p
        sc.F, sc.N, sc.D, sc.frames, sc.ragged = f, N, D, list(frames), len(set(frames)) > 1
        sc.F_total, sc.f0 = F, f0s[p]
        sc.stages = RaggedOracleStages(f, N, D, dtype, base)
        sc.stages.set_layout(list(frames), p)
        sc._bf = stat_block_frames(frames)
        sc._gbuf, sc._cidx, sc._pad, sc._cat = {}, {}, {}, {}
        scs.append(sc)
    bf = scs[0]._bf
    pending = {}

    def gather_for(key):
        def _g(k, t, _key=key):
            return pending[_key]
        return _g

    def exchange(key, parts, counts):
        n_max = max(counts)
        from vidcom2_amd.sharded import pad_rows
        pending[key] = torch.stack([pad_rows(t, n_max).clone() for t in parts])
        outs = []
        for sc, t in zip(scs, parts):
            sc._gather = gather_for(key)
            outs.append(sc._gather_rows(key, t, counts).clone())
        assert all(torch.equal(o, outs[0]) for o in outs)
        return outs[0]

    R = F * N
    stats_all = exchange("stats", [sc.stages.chan_stats(xs) for sc, xs in zip(scs, shards)], [f // bf for f in frames])
    for sc in scs:
        sc.stages.select_channels(stats_all, R)
    csum_all = torch.stack([sc.stages.phase1(xs) for sc, xs in zip(scs, shards)])
    s_all = exchange("s", [sc.stages.phase2(xs, csum_all, R) for sc, xs in zip(scs, shards)], list(frames))
    res = []
    for sc, xs in zip(scs, shards):
        sc.stages.select(xs, s_all.reshape(-1), sc.f0)
        res.append(sc.finish())
    return res, scs


@pytest.mark.parametrize("case", [(8, 49, 64, "bf16", "drift", 3, (1, 7)), (11, 37, 64, "f16", "drift", 3, (4, 4, 3)),
                                  (13, 49, 64, "bf16", "drift", 3, (2, 2, 2, 2, 2, 2, 1)),
                                  (10, 169, 128, "f16", "drift", 3, (3, 3, 2, 2)), (7, 7, 64, "bf16", "drift", 3, (1,) * 7),
                                  (11, 37, 64, "bf16", "cancel", 3, (4, 4, 3)), (11, 37, 64, "f16", "iid", 3, (5, 1, 5))],
                         ids=lambda c: "x".join(map(str, c[:5])) + "-" + "+".join(map(str, c[6])))
def test_padded_exchanges_and_compaction_match_the_oracle(case):
    """The compressor's padding and compaction (_gather_rows) on logical CPU ranks, the all-gather replaced by a stack:
    channel set, budgets and kept indices are the whole-pass oracle's for every split."""
    F, N, D, dn, dist_name, seed, frames = case
    x = synth.make(F, N, D, DTYPES[dn], seed, dist_name)
    ref = O.compress_indices(x, N, 0.25)
    res, scs = _emulate_cpu(x, frames, N, D, DTYPES[dn], 0.25)
    for sc in scs:
        assert sorted(sc.stages.chan_idx.tolist()) == sorted(ref["chan_idx"].tolist())
    assert torch.cat([r.ks for r in res]).tolist() == ref["ks"].tolist()
    assert torch.cat([r.global_idx for r in res]).tolist() == ref["global_idx"].tolist()


@pytest.mark.parametrize("F_total,world", [(100, 8), (77, 4), (5, 5), (3000, 7), (512, 8), (500, 8), (17, 2), (9, 4)])
def test_shard_frames(F_total, world):
    parts = shard_frames(F_total, world)
    assert len(parts) == world and sum(parts) == F_total and min(parts) >= 1
    if F_total >= 8 * world:
        assert all(p % 8 == 0 for p in parts[:-1])
        assert max(parts[:-1]) - min(parts[:-1]) <= 8                  # balanced in units of `align`
    else:
        assert max(parts) - min(parts) <= 1
    assert shard_frames(F_total, world, align=1) == [F_total // world + (1 if p < F_total % world else 0)
                                                     for p in range(world)]


def test_shard_frames_refuses_more_ranks_than_frames():
    with pytest.raises(ValueError):
        shard_frames(4, 5)
    assert shard_frames(512, 8) == [64] * 8
    assert shard_frames(100, 8) == [16, 16, 16, 16, 8, 8, 8, 12]
    assert stat_block_frames([8, 16]) == 8 and stat_block_frames([5, 19]) == 1 and stat_block_frames([4, 12, 6]) == 2


def _ctor_worker(rank, world, port, kind, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        N, D, dtype = 49, 64, torch.bfloat16
        if kind == "N":
            N += rank
        elif kind == "D":
            D += 2 * rank
        elif kind == "dtype":
            dtype = (torch.bfloat16, torch.float16)[rank]
        F = 2 + rank
        stages = OracleStages(F, N, D, dtype, 0.25) if kind == "no-layout-method" else RaggedOracleStages(F, N, D, dtype, 0.25)
        try:
            ShardedCompressor(F, N, D, dtype, "cpu", 0.25, stages=stages)
            q.put((rank, "accepted", ""))
        except Exception as e:                                          # noqa: BLE001 (the parent judges the type)
            q.put((rank, type(e).__name__, str(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind,error", [("N", "ValueError"), ("D", "ValueError"), ("dtype", "ValueError"),
                                        ("no-layout-method", "TypeError"), ("ok", "accepted")])
def test_constructor_checks_across_ranks(kind, error):
    """Unequal N, D or dtype still raise ValueError on every rank; unequal frame counts are accepted -- unless the injected
    stage object has no set_layout method to take the layout with."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ctor_worker, args=(r, world, port, kind, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=120) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert [g[1] for g in got] == [error] * world, got
    if kind == "no-layout-method":
        assert all("set_layout" in g[2] and "OracleStages" in g[2] for g in got)


# ---- GPU -----------------------------------------------------------------------------------------------------------

class _Spy:
    """A library handle that records which entry points a HipStages calls."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vc2_"):
            return fn

        def call(*a):
            self._log.append((name, a))
            return fn(*a)
        return call


def _spy_into(log):
    def spy(stages):
        stages._L = _Spy(stages._L, log)
    return spy


_REF = {}


def _reference(F, N, D, dn, seed, base, mode):
    """Input, oracle result ('torch' mode) and the unsharded HIP pass in library mode `mode`, once per case."""
    import vidcom2_amd as vc
    from vidcom2_amd import _ffi
    key = (F, N, D, dn, seed, base, mode)
    if key not in _REF:
        if len(_REF) > 2:
            _REF.clear()
        x = synth.make(F, N, D, DTYPES[dn], seed, "drift")
        xd = x.to("cuda:0")
        O.set_mode("torch")
        try:
            ref = O.compress_indices(x, N, base)
        finally:
            O.set_mode("exact")
        try:
            if mode == 2:
                assert _ffi.lib().vc2_set_mode(2) == 0
            whole = vc.compress(xd, N, base, want_scores=True)
            total = (whole.v_score + whole.f_score).float().flatten().clone()
            rows, gidx = whole.rows.clone(), whole.global_idx.clone()
        finally:
            _ffi.set_mode("torch")
        _REF[key] = (x, xd, ref, total, rows, gidx)
    return _REF[key]


MODE2_CASES = [(8, 49, 64, "bf16", (3, 5)), (8, 49, 64, "bf16", (1, 7)), (8, 49, 64, "bf16", (3, 2, 3)),
               (12, 5, 128, "f16", (1, 2, 3, 6)), (12, 5, 128, "f16", (5, 1, 1, 5)),
               (6, 3, 64, "bf16", (1, 1, 4)), (6, 3, 64, "bf16", (2, 1, 3)),
               (10, 100, 256, "bf16", (3, 7)), (10, 100, 256, "bf16", (4, 4, 2)),
               (6, 49, 64, "bf16", (1, 5), 8), (6, 49, 64, "bf16", (2, 1, 3), 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", MODE2_CASES,
                         ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[4])) + ("-cap8" if len(c) > 5 else ""))
def test_video_centre_replay_across_unequal_ranks(case):
    """Debug mode 2 flags EVERY video-centre column, so all of them go through exchange 2b in its ragged form: 16-row
    blocks straddle unequal ranks, ranks smaller than a block sit between larger ones; with vc_cap = 8 the rounds path
    runs.  Token by token the sharded scores are the unsharded pass's (same mode), the kept indices the oracle's."""
    from vidcom2_amd import _ffi
    F, N, D, dn, frames = case[:5]
    cap = case[5] if len(case) > 5 else D // 2
    dev = torch.device("cuda:0")
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 2, 0.25, 2)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    log = []
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        res, st, _ = emulate_ragged_ranks(xd, list(frames), N, D, DTYPES[dn], 0.25, dev, vc_cap=cap, spy=_spy_into(log))
    finally:
        _ffi.set_mode("torch")
    called = {n for n, _ in log}
    assert "vc2_video_centre_blocks_ragged" in called and "vc2_video_centre_blocks" not in called
    assert "vc2_video_centre_finish_round_ragged" in called          # (mode 2 goes in rounds, one or more)
    if len(case) > 5:
        assert "vc2_video_centre_blocks_round_ragged" in called       # more flagged columns than one exchange carries
    assert all(s.vc_fragile == 0 for s in st)
    assert torch.equal(torch.cat([s.total for s in st]), total)
    assert torch.equal(torch.cat([r.global_idx for r in res]).cpu(), ref["global_idx"])


DEFAULT_CASES = [(16, 169, 512, "f16", 0.15, (5, 11)), (16, 169, 512, "f16", 0.15, (7, 2, 7)),
                 (16, 196, 1024, "f32", 0.25, (5, 11)),
                 (24, 196, 3584, "bf16", 0.25, (8, 16)), (24, 196, 3584, "bf16", 0.25, (5, 19))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEFAULT_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[5])))
def test_unequal_shards_equal_the_unsharded_pass(case):
    """Default mode, warnings as errors: scores, budgets, kept indices and kept rows of unequal shards are the unsharded
    pass's and the oracle's.  fp32 has no replay (exchanges 1-3 only)."""
    F, N, D, dn, base, frames = case
    dev = torch.device("cuda:0")
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 1, base, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res, st, ex = emulate_ragged_ranks(xd, list(frames), N, D, DTYPES[dn], base, dev, spy=_spy_into(log))
    called = {n for n, _ in log}
    if dn != "f32":
        assert {"vc2_video_centre_blocks_ragged", "vc2_scores_phase2_blocks_ragged"} <= called
        assert all(s.vc_fragile == 0 for s in st)
        assert torch.equal(torch.cat([s.total for s in st]), total)
    else:
        assert not called & set(RAGGED_SYMBOLS)
    assert torch.cat([r.ks for r in res]).cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(torch.cat([r.global_idx for r in res]).cpu(), ref["global_idx"])
    assert all(torch.equal(s.mask, st[0].mask) for s in st)
    assert torch.equal(torch.cat([r.rows for r in res]), rows)
    assert torch.equal(torch.cat([r.rows for r in res]).cpu(), x[ref["global_idx"]])
    if frames == (8, 16):
        # multiples of 8 frames: the stat blocks stay at 8 frames and are, bit for bit, those of one logical rank
        assert all(s.bf == 8 for s in st) and ex["stats"].shape[0] == 3
        _, st1, ex1 = emulate_ragged_ranks(xd, [F], N, D, DTYPES[dn], base, dev)
        assert st1[0].bf == 8 and torch.equal(ex["stats"], ex1["stats"].reshape(-1, 2, D))


@pytest.mark.gpu
def test_half_a_million_rows_over_two_unequal_ranks():
    """2688 x 196 x 64 bf16 split (1000, 1688): R_total > 2^19, so torch's level_power is 5 and the level-0 blocks are 32
    rows.  Debug mode 2 (every column through the ragged exchange 2b), against the unsharded pass in the same mode and
    the oracle (0.4 s on the CPU at this width)."""
    from vidcom2_amd import _ffi
    F, N, D, frames = 2688, 196, 64, [1000, 1688]
    assert F * N > 1 << 19
    dev = torch.device("cuda:0")
    x, xd, ref, total, rows, gidx = _reference(F, N, D, "bf16", 1, 0.25, 2)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        res, st, _ = emulate_ragged_ranks(xd, frames, N, D, torch.bfloat16, 0.25, dev)
    finally:
        _ffi.set_mode("torch")
    assert all(s.vc_fragile == 0 for s in st)
    assert torch.equal(torch.cat([s.total for s in st]), total)
    assert torch.cat([r.ks for r in res]).cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(torch.cat([r.global_idx for r in res]).cpu(), ref["global_idx"])
    assert torch.equal(torch.cat([r.rows for r in res]), rows)


@pytest.mark.gpu
def test_real_collective_with_unequal_shards():
    """Two processes share cuda:0 over gloo, one with 5 frames and one with 3 of 8 x 49 x 64 bf16: ShardedCompressor, the
    HIP stages and a real (padded) collective.  Each child runs under its own time limit; nothing is started after a
    failure."""
    import vidcom2_amd as vc
    import tempfile
    frames = (5, 3)
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    with tempfile.TemporaryDirectory() as tmp:
        outs = [os.path.join(tmp, f"rank{r}.pt") for r in range(2)]
        procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_ragged_shards.py"),
                                   str(r), ",".join(map(str, frames)), str(port), outs[r]], env=env, cwd=ROOT,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
        logs = [p.communicate()[0] for p in procs]                      # (the ranks need each other: started together)
        codes = [p.returncode for p in procs]
        assert codes == [0, 0], (codes, [lg[-2000:] for lg in logs])
        got = [torch.load(o) for o in outs]
    x = synth.make(8, 49, 64, torch.bfloat16, 2, "drift")
    whole = vc.compress(x.to("cuda:0"), 49, 0.25)
    assert torch.equal(torch.cat([g["gidx"] for g in got]), whole.global_idx.cpu())
    assert torch.equal(torch.cat([g["ks"] for g in got]), whole.ks.cpu())
    assert torch.equal(torch.cat([g["rows"] for g in got]), whole.rows.cpu())
    assert all(torch.equal(g["all"], whole.global_idx.cpu()) for g in got)
    assert [g["ks"].numel() for g in got] == list(frames)


@pytest.mark.gpu
def test_split_invariance():
    """One video, three different splits (and the equal one): identical channel mask, scores and kept indices."""
    F, N, D = 13, 49, 64
    dev = torch.device("cuda:0")
    xd = synth.make(F, N, D, torch.bfloat16, 4, "drift").to(dev)
    outs = []
    for frames in ([5, 8], [1, 6, 6], [4, 3, 2, 4], [13]):
        res, st, _ = emulate_ragged_ranks(xd, frames, N, D, torch.bfloat16, 0.25, dev)
        assert all(torch.equal(s.mask, st[0].mask) for s in st)
        outs.append((st[0].mask.clone(), torch.cat([s.total for s in st]), torch.cat([r.global_idx for r in res])))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.gpu
def test_equal_layout_goes_through_the_equal_rank_entry_points():
    """An equal layout -- handed over as a layout or not -- issues the calls it always did: the same entry points with the
    same arguments, none of the ragged symbols."""
    F, N, D, P = 8, 49, 64, 2
    dev = torch.device("cuda:0")
    xd = synth.make(F, N, D, torch.bfloat16, 2, "drift").to(dev)
    log_a, log_b = [], []
    res_a, st_a, _ = emulate_ragged_ranks(xd, [F // P] * P, N, D, torch.bfloat16, 0.25, dev, spy=_spy_into(log_a))
    from test_sharded import _emulate_ranks_on_one_gpu
    from vidcom2_amd.sharded import HipStages
    made = []
    orig = HipStages.__init__

    def init(self, *a, **k):
        orig(self, *a, **k)
        _spy_into(log_b)(self)
        made.append(self)
    HipStages.__init__ = init
    try:
        res_b, st_b = _emulate_ranks_on_one_gpu(xd, F, N, D, torch.bfloat16, 0.25, P, dev)
    finally:
        HipStages.__init__ = orig
    assert not {n for n, _ in log_a} & set(RAGGED_SYMBOLS)
    assert not any(s.ragged for s in st_a)
    assert [n for n, _ in log_a] == [n for n, _ in log_b]

    def plain(args):                                                   # sizes and flags; buffers differ between the two runs
        return [a for a in args if isinstance(a, (int, float))]
    assert [plain(a) for _, a in log_a] == [plain(a) for _, a in log_b]
    assert torch.equal(torch.cat([r.global_idx for r in res_a]), torch.cat([r.global_idx for r in res_b]))

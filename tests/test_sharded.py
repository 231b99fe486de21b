"""Frame-sharded path.  CPU: world_size-2 gloo run of the collective logic with the
oracle-backed stages.  GPU: P = 1, 2, 4 logical ranks on one device through the HIP stage entry
points -- results must not depend on the world size and must equal the unsharded pass."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import oracle as O
from vidcom2_amd import synth
from vidcom2_amd.sharded import ShardedCompressor

from _oracle_stages import OracleStages

SHAPE = (8, 49, 64, 0.25)      # F_total, N, D, base


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, dtype_name, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, base = SHAPE
        dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[dtype_name]
        x = synth.make(F, N, D, dtype, 3, "drift")
        Fl = F // world
        xl = x[rank * Fl * N: (rank + 1) * Fl * N].contiguous()
        sc = ShardedCompressor(Fl, N, D, dtype, "cpu", base, stages=OracleStages(Fl, N, D, dtype, base))
        res = sc(xl)
        # SURVEY §8e "output": every rank (or one) can also get ALL kept rows, in frame order
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert counts[rank] == res.K and torch.equal(rows_all, x[gidx_all])
        only0 = sc.gather_kept(res, dst=0)
        assert (only0 is None) == (rank != 0)
        q.put((rank, res.global_idx.tolist(), res.ks.tolist(), synth.sha256_tensor(res.rows)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype_name", ["bf16", "f32"])
def test_gloo_world2_matches_unsharded(dtype_name):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, dtype_name, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    F, N, D, base = SHAPE
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32}[dtype_name]
    x = synth.make(F, N, D, dtype, 3, "drift")
    ref = O.compress_indices(x, N, base)
    gidx = sum((g[1] for g in got), [])
    ks = sum((g[2] for g in got), [])
    assert ks == ref["ks"].tolist()
    assert gidx == ref["global_idx"].tolist()
    # each rank's rows are the kept rows of its own frames
    for r, gi, _, sha in got:
        assert synth.sha256_tensor(x[torch.tensor(gi, dtype=torch.int64)]) == sha


def _emulate_ranks_on_one_gpu(x, F, N, D, dtype, base, P, dev, vc_cap=64):
    """P logical ranks, one HipStages each, exchanges done by stacking (what all_gather returns)."""
    from vidcom2_amd.sharded import HipStages
    Fl = F // P
    shards = [x[p * Fl * N: (p + 1) * Fl * N].contiguous() for p in range(P)]
    st = [HipStages(Fl, N, D, dtype, dev, base, vc_cap=vc_cap) for _ in range(P)]
    for s_ in st:
        s_.F_total = F
    stats_all = torch.stack([s.chan_stats(xs).clone() for s, xs in zip(st, shards)])
    for s in st:
        s.select_channels(stats_all, F * N)
    csum_all = torch.stack([s.phase1(xs).clone() for s, xs in zip(st, shards)])
    blocks = [s.vc_blocks(xs, csum_all, F * N, p * Fl) for p, (s, xs) in enumerate(zip(st, shards))]   # exchange 2b (may not apply)
    if all(b is not None for b in blocks) and st[0].needs_rounds():
        # proven / debug modes: rounds of exchange 2b, all ranks in lock step (ShardedCompressor._enqueue)
        counts = [s.flagged_columns() for s in st]
        assert len(set(counts)) == 1, counts
        for j0 in range(0, max(counts[0], 1), st[0].vc_cap):
            if j0:
                blocks = [s.vc_blocks_round(xs, F * N, p * Fl, j0) for p, (s, xs) in enumerate(zip(st, shards))]
            blocks_all = torch.stack([b.clone() for b in blocks])
            for s in st:
                s.vc_finish_round(F * N, blocks_all, j0)
        s_all = torch.cat([s.phase2(xs, csum_all, F * N, vc_final=True).clone() for s, xs in zip(st, shards)])
    elif all(b is not None for b in blocks):
        blocks_all = torch.stack([b.clone() for b in blocks])
        s_all = torch.cat([s.phase2(xs, csum_all, F * N, blocks_all).clone() for s, xs in zip(st, shards)])
    else:
        s_all = torch.cat([s.phase2(xs, csum_all, F * N).clone() for s, xs in zip(st, shards)])
    out = []
    for p, (s, xs) in enumerate(zip(st, shards)):
        s.select(xs, s_all, p * Fl)
        out.append(s.result(p * Fl))
    return out, st


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(8, 49, 64, "bf16", 0.25), (16, 196, 1024, "bf16", 0.25), (16, 196, 1024, "f32", 0.25),
                                  (32, 196, 3584, "bf16", 0.25), (16, 169, 512, "f16", 0.15)],
                         ids=lambda c: "x".join(map(str, c)))
def test_world_size_invariance_on_gpu(case):
    import vidcom2_amd as vc
    F, N, D, dn, base = case
    dtype = {"bf16": torch.bfloat16, "f32": torch.float32, "f16": torch.float16}[dn]
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, dtype, 1, "drift")
    xd = x.to(dev)
    O.set_mode("torch")
    ref = O.compress_indices(x, N, base)
    O.set_mode("exact")
    whole = vc.compress(xd, N, base, want_scores=True)
    assert torch.equal(whole.global_idx.cpu(), ref["global_idx"])
    import warnings
    for P in (1, 2, 4):
        with warnings.catch_warnings():
            warnings.simplefilter("error")       # (no "could not be replayed across ranks": 169-token frames included)
            res, st = _emulate_ranks_on_one_gpu(xd, F, N, D, dtype, base, P, dev)
        if dtype != torch.float32:
            # every boundary-near video-centre mean was replayed across the ranks -- also where a rank's row count is
            # not a multiple of the cascade's 16-row blocks (169-token frames) --: the scores themselves are the
            # unsharded pass's bits, not only the decisions taken from them
            assert all(s.vc_fragile == 0 for s in st)
            tot = torch.cat([s.total for s in st])
            assert torch.equal(tot, (whole.v_score + whole.f_score).float().flatten()), f"P={P}"
        gidx = torch.cat([r.global_idx for r in res]).cpu()
        ks = torch.cat([r.ks for r in res]).cpu()
        assert ks.tolist() == ref["ks"].tolist(), f"P={P}"
        assert torch.equal(gidx, ref["global_idx"]), f"P={P}"
        assert all(torch.equal(s.mask, st[0].mask) for s in st)
        rows = torch.cat([r.rows for r in res])
        assert torch.equal(rows, whole.rows)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(6, 49, 64, "bf16", (2, 3)), (12, 169, 128, "f16", (2, 3, 4, 6)), (10, 100, 256, "bf16", (2, 5)),
                                  (9, 37, 64, "f16", (3,)),
                                  # ranks with FEWER rows than a 16-row cascade block: a block meets three and more ranks
                                  (8, 7, 64, "bf16", (2, 4, 8)), (12, 5, 128, "f16", (3, 6, 12)), (6, 3, 64, "bf16", (6,)),
                                  # more flagged columns than one exchange carries: rounds (cap 8 of 32 / 64 columns)
                                  (6, 49, 64, "bf16", (2, 3), 8), (10, 100, 128, "f16", (2, 5), 8)],
                         ids=lambda c: "x".join(map(str, c[:4])) + ("-cap%d" % c[5] if len(c) > 5 else ""))
def test_video_centre_replay_across_unaligned_ranks(case):
    """Debug mode 2 flags EVERY video-centre column, so all of them go through exchange 2b: ranks whose row count is
    not a multiple of 16 share level-0 blocks with their neighbours (raw head / tail values in the record), and a video
    whose row count is not a multiple of 16 ends in the cascade's tail rows.  Token by token the sharded scores must be
    the unsharded pass's (same mode) and the oracle's."""
    import vidcom2_amd as vc
    from vidcom2_amd import _ffi
    F, N, D, dn, worlds = case[:5]
    cap = case[5] if len(case) > 5 else D // 2
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dn]
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, dtype, 2, "drift")
    xd = x.to(dev)
    O.set_mode("torch")
    ref = O.compress_indices(x, N, 0.25)
    O.set_mode("exact")
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        whole = vc.compress(xd, N, 0.25, want_scores=True)
        assert torch.equal(whole.v_score.cpu().float(), ref["v"].float()) and torch.equal(whole.global_idx.cpu(), ref["global_idx"])
        total = (whole.v_score + whole.f_score).float().flatten()
        for P in worlds:
            res, st = _emulate_ranks_on_one_gpu(xd, F, N, D, dtype, 0.25, P, dev, vc_cap=cap)
            assert all(s.vc_fragile == 0 for s in st), f"P={P}"
            assert torch.equal(torch.cat([s.total for s in st]), total), f"P={P}"
            assert torch.equal(torch.cat([r.global_idx for r in res]).cpu(), ref["global_idx"]), f"P={P}"
    finally:
        _ffi.set_mode("torch")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(32, 196, 3584, "bf16", "iid"), (16, 169, 1024, "f16", "iid"), (16, 196, 1024, "bf16", "cancel")],
                         ids=lambda c: "x".join(map(str, c)))
def test_proven_margin_mode_sharded_goes_in_rounds(case):
    """Mode 3 (proven centre margins) flags hundreds of video-centre columns on zero-mean data -- far more than one
    exchange 2b carries (64): the sharded pass then goes in rounds and must still give the unsharded pass's bits, with no
    column left at its exactly rounded mean (until round 4 those were counted and warned about)."""
    import warnings
    import vidcom2_amd as vc
    from vidcom2_amd import _ffi
    F, N, D, dn, dist_ = case
    dtype = {"bf16": torch.bfloat16, "f16": torch.float16}[dn]
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, dtype, 5, dist_)
    xd = x.to(dev)
    try:
        _ffi.set_mode("torch_proven")
        whole = vc.compress(xd, N, 0.25, want_scores=True)
        total = (whole.v_score + whole.f_score).float().flatten()
        for P in (2, 4):
            with warnings.catch_warnings():
                warnings.simplefilter("error")
                res, st = _emulate_ranks_on_one_gpu(xd, F, N, D, dtype, 0.25, P, dev)
            assert st[0].needs_rounds()
            assert all(s.vc_fragile == 0 for s in st), f"P={P}"
            assert torch.equal(torch.cat([s.total for s in st]), total), f"P={P}"
            assert torch.equal(torch.cat([r.global_idx for r in res]), whole.global_idx), f"P={P}"
    finally:
        _ffi.set_mode("torch")


@pytest.mark.gpu
def test_sharded_compressor_single_process():
    """world_size 1 (no process group): the ShardedCompressor object itself == the fused pass."""
    import vidcom2_amd as vc
    dev = torch.device("cuda:0")
    x = synth.make(32, 196, 3584, torch.bfloat16, 0, "drift").to(dev)
    sc = ShardedCompressor(32, 196, 3584, torch.bfloat16, dev, 0.25)
    r = sc(x)
    w = vc.compress(x, 196, 0.25)
    assert torch.equal(r.global_idx, w.global_idx) and torch.equal(r.ks, w.ks) and torch.equal(r.rows, w.rows)


def _gpu_worker(rank, world, port, q):
    """world_size-2 process group whose ranks share cuda:0 (RCCL refuses two ranks on one device -- 'Duplicate GPU
    detected' -- so the collectives run on gloo, which stages device tensors through the host): the REAL HIP stages
    driven by ShardedCompressor through a REAL collective."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        F, N, D, base = 16, 196, 1024, 0.25
        dev = torch.device("cuda:0")
        x = synth.make(F, N, D, torch.bfloat16, 2, "drift")
        Fl = F // world
        xl = x[rank * Fl * N: (rank + 1) * Fl * N].contiguous().to(dev)
        sc = ShardedCompressor(Fl, N, D, torch.bfloat16, dev, base)
        res = sc(xl)
        torch.cuda.synchronize()
        rows_all, gidx_all, counts = sc.gather_kept(res)
        assert sum(counts) == rows_all.shape[0] and torch.equal(rows_all.cpu(), x[gidx_all.cpu()])
        q.put((rank, res.global_idx.cpu().tolist(), res.ks.cpu().tolist(), synth.sha256_tensor(res.rows.cpu())))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
def test_two_processes_one_gpu_hip_stages_and_a_real_collective():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=300) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:                                           # (a stuck rank must not outlive the test)
            if p.is_alive():
                p.kill()
    F, N, D, base = 16, 196, 1024, 0.25
    x = synth.make(F, N, D, torch.bfloat16, 2, "drift")
    O.set_mode("torch")
    ref = O.compress_indices(x, N, base)
    O.set_mode("exact")
    assert sum((g[2] for g in got), []) == ref["ks"].tolist()
    assert sum((g[1] for g in got), []) == ref["global_idx"].tolist()
    for r, gi, _, sha in got:
        assert synth.sha256_tensor(x[torch.tensor(gi, dtype=torch.int64)]) == sha


@pytest.mark.gpu
def test_bench_two_rank_code_path_on_one_gpu():
    """bench.py --gpus 2 end to end (ShardedCompressor + the four exchanges + timing + the JSON line), both ranks on
    cuda:0 with gloo collectives (RCCL refuses two ranks on one device): the code the driver's scaling run executes."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VC2_BENCH_ONE_GPU="1", VC2_BENCH_BACKEND="gloo", VC2_BENCH_CPU_THREADS="16,32")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3",
           "--warmup", "1", "--workload", "cfg2"]
    out = _run_bounded(cmd, env, root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                   # rank 0 prints exactly one JSON line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["value"] > 0 and d["config"]["parallelism"] == "frame-shard x2"


def _run_bounded(cmd, env, cwd, timeout=420):
    """subprocess.run for the multi-process bench runs, bounded: its own session (a timeout kills the launcher AND its
    ranks -- an orphaned rank would keep the pipes open and block communicate() for good) and bench.py's watchdog (every
    thread's Python stack on stderr when a rank is still going after timeout - 120 s).  A run cut off either way fails
    the test with the stderr it collected; an ordinary failure is returned as is."""
    import signal
    import subprocess
    env = dict(env, VC2_BENCH_WATCHDOG=str(max(60, timeout - 120)))
    p = subprocess.Popen(cmd, env=env, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         start_new_session=True)
    try:
        out, err = p.communicate(timeout=timeout)
        cut = p.returncode != 0 and "Timeout (" in err                  # (faulthandler's watchdog header)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        out, err = p.communicate()
        err = f"[cut off after {timeout} s]\n" + err
        cut = True
    if cut:
        pytest.fail(f"bench subprocess was cut off by its watchdog / timeout:\n{err[-3000:]}")
    return subprocess.CompletedProcess(cmd, p.returncode, out, err)


def _run_bench(args, env_extra=None, timeout=600):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VC2_BENCH_CPU_THREADS="16,32", **(env_extra or {}))
    out = _run_bounded([sys.executable, os.path.join(root, "bench.py")] + args, env, root, timeout=timeout)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    return out, (json.loads(lines[0]) if len(lines) == 1 else None)


@pytest.mark.gpu
def test_bench_sharded_pass_on_rccl_at_world_one():
    """VC2_BENCH_FORCE_DIST=1: the frame-sharded pass with its four all-gathers on the `nccl` (= RCCL) backend, one
    rank -- all_gather_into_tensor on fp64 / fp32 device tensors really executes -- behind the CPU parity gate; the
    line reports the GPU count it ran on and the time of every exchange."""
    out, d = _run_bench(["--gpus", "1", "--workload", "cfg2", "--steps", "3", "--warmup", "1", "--full", "--no-extra"],
                        {"VC2_BENCH_FORCE_DIST": "1", "MASTER_PORT": str(_free_port())})
    assert out.returncode == 0, out.stderr[-2000:]
    assert d is not None and d["n_gpus"] == 1 and d["config"]["parallelism"] == "frame-shard x1"
    assert d["cpu_baseline"] is not None                      # the parity gate ran (and passed) on the sharded result
    ex = d["exchanges_us"]
    assert set(ex) >= {"stats", "csum", "s"} and all(v["us"] > 0 and v["bytes_per_rank"] > 0 for v in ex.values())


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_only(tmp_path):
    """Without --full a run times the steps, dumps the last step's outputs and prints the line: the contract's fields,
    no parity gate, CPU baselines, per-kernel or side legs."""
    out, d = _run_bench(["--gpus", "1", "--workload", "cfg2", "--steps", "3", "--warmup", "1",
                         "--dump-outputs", str(tmp_path)])
    assert out.returncode == 0, out.stderr[-2000:]
    assert d is not None and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "tokens/s"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["steps"] == 3 and d["warmup"] == 1
    assert d["cpu_baseline"] is None and d["roofline"] is None
    assert not {"kernels_us", "median_ms_per_step", "hipgraph_replay", "cfg3"} & set(d)
    assert {p.name for p in tmp_path.iterdir()} == {"rows.npy", "global_idx.npy", "ks.npy"}


@pytest.mark.gpu
def test_bench_refuses_more_gpus_than_the_node_has():
    """`python bench.py --gpus N` without a launcher spawns its own ranks -- and must not print a line when the node
    has fewer devices (round 2: it silently ran on one GPU)."""
    import torch as _t
    n = _t.cuda.device_count() + 1
    out, d = _run_bench(["--gpus", str(n), "--steps", "2", "--warmup", "1", "--no-extra", "--no-cpu-baseline"])
    assert out.returncode != 0 and d is None and "refusing" in (out.stderr + out.stdout)
    # and under a launcher the line's n_gpus cannot differ from --gpus
    out, d = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--no-extra", "--no-cpu-baseline"],
                        {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert out.returncode != 0 and d is None


@pytest.mark.gpu
def test_bench_cfg4_strong_scaling_two_ranks_on_one_gpu():
    """BASELINE configs[3] (one 512-frame video, frame-sharded: 256 frames per rank here) through bench.py's own code
    path: two ranks on cuda:0 with gloo collectives."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, VC2_BENCH_ONE_GPU="1", VC2_BENCH_BACKEND="gloo", VC2_BENCH_CPU_THREADS="16,32")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--workload", "cfg4"]
    out = _run_bounded(cmd, env, root)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["frames_per_gpu"] == 256
    assert d["config"]["workload"].startswith("cfg4: 512 frames")


@pytest.mark.gpu
def test_bench_cfg5_replicas():
    """BASELINE configs[4]: 16 clips, replicas, no collective; parity gate on clip 0."""
    out, d = _run_bench(["--gpus", "1", "--workload", "cfg5", "--steps", "1", "--warmup", "1", "--full"])
    assert out.returncode == 0, out.stderr[-2000:]
    assert d["n_gpus"] == 1 and d["config"]["parallelism"] == "replicas x1" and d["dtype"] == "f16" and d["value"] > 0

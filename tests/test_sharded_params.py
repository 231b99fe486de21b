"""Pass parameters (channel ratio, softmax temperature, Gaussian scales) in the frame-sharded pass, and the replay of the
video centre's C % 32 tail columns (row_sum's four interleaved chains) across ranks.  CPU: the constructor's checks over
gloo, a world-3 run with parameter-honouring oracle stages, the host arithmetic of the tail record.  GPU: logical ranks
on one device through the `_o` entry points against the reference's recorded values, the unsharded pass and the oracle.

score_dtype=torch.float32 over bf16 / fp16 rows: the sharded pass against tests/golden/score_dtype_cases.json and the
unsharded fp32-scored pass."""
import ctypes
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import PassParams, synth
from vidcom2_amd.sharded import HipStages, ShardedCompressor, tail_columns

from _ragged_shards import DTYPES
from _sharded_params import (GPU_CHILD_PARAMS, ctor_worker, emulate_ranks, four_chain_sum, gloo_worker, params_of,
                             tail_finish, tail_record_plan, tail_records)
from _stage_chain import digest
import _score_dtype as SD
from conftest import load_json, make_input
from test_ragged_shards import _free_port, _spy_into

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OWN = load_json("pass_params_cases.json")["cases"]


def own_case(name, F, N, D, dn):
    (c,) = [c for c in OWN if (c["name"], c["F"], c["N"], c["D"], c["dtype"]) == (name, F, N, D, dn)]
    return c


# ---- CPU -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,error", [("params", "ValueError"), ("temp", "ValueError"), ("alphas", "ValueError"),
                                        ("none-vs-set", "ValueError"), ("score_dtype", "ValueError"),
                                        ("equal", "accepted"), ("default-vs-none", "accepted"), ("score-equal", "accepted"),
                                        ("score-plain", "accepted")])
def test_constructor_compares_params_and_score_dtype_across_ranks(kind, error):
    """Ranks whose params or score_dtype differ raise ValueError on EVERY rank; equal sets -- a default-equal PassParams
    beside None, score_dtype == dtype beside None included -- are accepted (injected CPU stages)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=ctor_worker, args=(r, world, port, kind, q)) for r in range(world)]
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
    if error == "ValueError":
        assert all("same params and score_dtype" in g[2] for g in got)


def test_gloo_world3_with_params_matches_the_reference():
    """Three gloo ranks (3, 2, 3) with oracle stages that honour ratio 0.25, temp 0.05 and four scales: budgets and kept
    indices are the reference's recorded ones (fixture case llava_vid 8x169x1024 bf16: its linear-map values)."""
    c = own_case("llava_vid", 8, 169, 1024, "bf16")
    assert (c["ratio"], c["temp"], c["alphas"]) == (0.25, 0.05, [0.1, 0.3, 1.0, 3.0])
    frames = [3, 2, 3]
    world = len(frames)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    case = (c["F"], c["N"], c["D"], c["dtype"], c["seed"], c["dist"], c["base"])
    procs = [ctx.Process(target=gloo_worker, args=(r, frames, case, port, q)) for r in range(world)]
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
    assert sum((g[1] for g in got), []) == c["ks"]
    for g in got:
        assert len(g[2]) == c["K"] and digest(torch.tensor(g[2], dtype=torch.int64)) == c["keep_sha256"]


def test_tail_record_host_arithmetic():
    """The record FORMAT of a tail column as include/vc2.h states it (head / run / tail counts per rank, the owner of a video
    row), restated in the test helper: a finisher over such records gives the bits of a plain restatement of row_sum's four
    interleaved chains, over random splits -- ranks smaller than a run, a video smaller than a run, runs of 64 rows.  (The
    kernels' own counts are covered by the GPU tests in debug mode 2, not here.)"""
    rng = random.Random(7)
    nrng = np.random.default_rng(7)
    assert tail_columns(50) == 18 and tail_columns(7) == 3 and tail_columns(36) == 4 and tail_columns(28) == 28
    assert tail_columns(1792) == 0 and tail_columns(1075) == 19 and tail_columns(4) == 0
    for R in (18, 63, 64, 350, 1001, 2500):
        vals = (nrng.standard_normal(R) * 0.05).astype(np.float32)
        want = four_chain_sum(vals)
        for _ in range(6):
            world = rng.randint(1, min(6, R))
            cuts = sorted(rng.sample(range(1, R), world - 1))
            rows = [b - a for a, b in zip([0] + cuts, cuts + [R])]
            recs, plan, run = tail_records(vals, rows)
            assert run == 64
            assert sum(h + r * run + t for _, h, r, t in plan) == R
            for (row0, h, r, t), n in zip(plan, rows):
                assert 0 <= h < run and 0 <= t < run and (h == n or (row0 + h) % run == 0)
                assert r == ((row0 + n) // run - (row0 + run - 1) // run if h < n else 0)
            got = tail_finish(recs, plan, run, R)
            assert got.tobytes() == want.tobytes(), (R, rows)
    # beyond 2^21 rows the chains of R / 4 cascade at level power 5: runs of 128 rows; up to 2^21, 64 although the plain
    # columns' level power is already 5 above 2^19
    assert tail_record_plan([1 << 20, 1 << 20])[1] == 64 and tail_record_plan([(1 << 21) + 4])[1] == 128
    assert tail_record_plan([196000, 330848])[0] == [(0, 0, 3062, 32), (196000, 32, 5169, 0)]


def test_stage_buffers_and_options_follow_the_params():
    """HipStages' host side (buffers on the CPU, no launch): C, the record stride and the options of the `_o` forms follow
    params; defaults, a default-equal set and an empty tail leave the plain pass (no options, the narrow stride)."""
    def stages(D, dtype=torch.bfloat16, **kw):
        return HipStages(2, 50, D, dtype, "cpu", 0.25, **kw)
    for kw in ({}, {"params": PassParams()}, {"params": PassParams(0.5, 0.01, [0.125, 0.25, 0.5, 1.0, 2.0])},
               {"score_dtype": torch.bfloat16}):
        s = stages(128, **kw)
        assert (s.C, s.vc_tail, s._opts) == (64, False, None) and s.blocks.shape[1] == 2 * 64 + 1 + 100 // 16
        assert s.csum.shape[1] == 64
    s = stages(100)                                                    # default parameters, C = 50: 18 tail columns
    assert s.vc_tail and s._opts is not None and s._opts.params is None
    assert (s._opts.score_dtype, s._opts.tail_records) == (s.code, 1) and s.blocks.shape[1] == 2 * 256 + 1 + 100 // 16
    s = stages(128, params=PassParams(0.25, 0.05))                     # C = 32: parameters, empty tail
    assert (s.C, s.vc_tail, s.csum.shape[1]) == (32, False, 32) and s.blocks.shape[1] == 2 * 64 + 1 + 100 // 16
    assert s._opts.params == ctypes.addressof(s._cparams) and (s._opts.score_dtype, s._opts.tail_records) == (s.code, 0)
    s = HipStages(2, 50, 128, torch.bfloat16, "cpu", 0.25, frames=[2, 5], rank=0, params=PassParams(0.3))
    assert (s.C, s.vc_tail) == (38, True) and s.blocks.shape[1] == 2 * 256 + 1 + 250 // 16
    s = stages(64, torch.float32, params=PassParams(0.3))              # fp32 rows: no replay, so no tail records
    assert (s.C, s.vc_tail, s._opts.tail_records) == (19, False, 0)
    s = stages(100, score_dtype=torch.float32)                         # fp32 scoring: no replay, so no records either
    assert s.score32 and not s.vc_replay and not s.vc_tail and s._opts.params is None
    assert (s._opts.score_dtype, s._opts.tail_records) == (0, 0) and s.rows.dtype == torch.bfloat16
    with pytest.raises(ValueError):
        stages(64, score_dtype=torch.float16)
    with pytest.raises(ValueError):
        stages(64, params=PassParams(1 / 128))
    with pytest.raises(NotImplementedError):
        stages(8192, params=PassParams(1.0))


# ---- GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def _counters():
    from vidcom2_amd._ffi import check, lib
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 1), "vc2_selftest_counters")     # (reset: this module's hits only)
    yield
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)


@pytest.fixture
def _modes(_counters):
    from vidcom2_amd import _ffi
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("exact")


PARAM_CASES = [("rt", 12, 196, 1024, "bf16", (8, 4)), ("rt", 12, 196, 1024, "bf16", (5, 7)),
               ("rt", 6, 144, 1536, "bf16", (2, 4)),
               ("rta", 16, 324, 1536, "bf16", (8, 8)), ("rta", 16, 324, 1536, "bf16", (5, 11)),
               ("rta", 6, 144, 1536, "f16", (1, 2, 3)),
               ("a4", 12, 144, 1536, "f16", (4, 4, 4)),
               ("rta", 8, 196, 3584, "f16", (3, 5))]
_WHOLE = {}


def _whole(c, x):
    key = (c["name"], c["F"], c["N"], c["D"], c["dtype"])
    if key not in _WHOLE:
        if len(_WHOLE) > 1:
            _WHOLE.clear()
        w = vc.compress(x.to("cuda:0"), c["N"], c["base"], params=params_of(c), want_scores=True)
        _WHOLE[key] = ((w.v_score + w.f_score).float().flatten().clone(), w.ks.clone(), w.global_idx.clone(), w.rows.clone())
    return _WHOLE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARAM_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}-" + "+".join(map(str, c[5])))
def test_sharded_pass_with_params_equals_the_reference(case, _modes):
    """16-bit rows, "torch" mode, warnings as errors: budgets, kept indices and kept rows are the reference's recorded ones and
    the unsharded parametrised pass's; the scores are the unsharded pass's bit for bit; no video-centre value is left
    unreplayed (ratio 1/128 at 3584: C = 28, EVERY column is a tail column)."""
    name, F, N, D, dn, frames = case
    c = own_case(name, F, N, D, dn)
    x = make_input(F, N, D, dn, c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    dev = torch.device("cuda:0")
    total, ks, gidx, rows = _whole(c, x)
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res, st = emulate_ranks(x.to(dev), list(frames), N, D, DTYPES[dn], c["base"], dev, params=params_of(c),
                                spy=_spy_into(log))
    print(case, "C", st[0].C, "tail", tail_columns(st[0].C), "fragile", [s.vc_fragile for s in st],
          "ks", torch.cat([r.ks for r in res]).tolist(), "reference", c["ks"])
    assert st[0].C == int(D * (0.5 if c["ratio"] is None else c["ratio"]))
    assert all(n.endswith("_o") or n in ("vc2_chan_var_from_stats", "vc2_chan_select", "vc2_video_centre_flagged", "vc2_get_mode")
               for n, _ in log), {n for n, _ in log}
    assert all(s.vc_fragile == 0 for s in st)
    got_ks, got_idx = torch.cat([r.ks for r in res]), torch.cat([r.global_idx for r in res])
    got_rows = torch.cat([r.rows for r in res])
    assert got_ks.cpu().tolist() == c["ks"] and int(got_idx.numel()) == c["K"]
    assert digest(got_idx) == c["keep_sha256"] and digest(got_rows) == c["rows_sha256"]
    assert torch.equal(got_ks, ks) and torch.equal(got_idx, gidx) and torch.equal(got_rows, rows)
    assert torch.equal(torch.cat([s.total for s in st]), total)


_REF2 = {}


def _mode2_reference(F, N, D, dn, seed, params):
    """Input, the oracle's kept indices ("torch" mode, default parameters only) and the unsharded pass in debug mode 2."""
    from vidcom2_amd import _ffi
    key = (F, N, D, dn, seed, params)
    if key not in _REF2:
        if len(_REF2) > 1:
            _REF2.clear()
        x = synth.make(F, N, D, DTYPES[dn], seed, "drift")
        xd = x.to("cuda:0")
        ref = O.compress_indices(x, N, 0.25) if params is None else None
        try:
            assert _ffi.lib().vc2_set_mode(2) == 0
            whole = vc.compress(xd, N, 0.25, params=params, want_scores=True)
            total = (whole.v_score + whole.f_score).float().flatten().clone()
            gidx, rows = whole.global_idx.clone(), whole.rows.clone()
        finally:
            _ffi.set_mode("torch")
        _REF2[key] = (xd, ref, total, gidx, rows)
    return _REF2[key]


R716 = PassParams(7 / 16)
TAIL_CASES = [(7, 50, 100, "bf16", (3, 1, 3), None, None), (7, 50, 100, "bf16", (2, 5), None, None),
              (7, 50, 100, "f16", (3, 1, 3), None, None), (7, 50, 100, "f16", (2, 5), None, None),
              (6, 3, 16, "bf16", (1, 1, 4), R716, None),
              (9, 33, 72, "f16", (4, 5), None, None), (9, 33, 72, "f16", (3, 3, 3), None, None),
              (9, 33, 72, "f16", (4, 5), None, 2), (9, 33, 72, "f16", (3, 3, 3), None, 2),
              (8, 50, 100, "bf16", (4, 4), None, None), (6, 3, 16, "bf16", (2, 2, 2), R716, None)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[4]))
                         + ("-r7/16" if c[5] else "") + (f"-cap{c[6]}" if c[6] else ""))
def test_tail_columns_are_replayed_across_ranks(case, _modes):
    """Debug mode 2 flags EVERY video-centre column, so the C % 32 tail columns go through exchange 2b in the wide record
    layout: 64-row runs straddle ranks, a 50-row rank sits inside one run, 18 rows are all raw; with vc_cap = 2 plain and
    tail columns go in separate rounds.  Token by token the sharded scores are the unsharded pass's (same mode), the kept
    indices the oracle's; nothing stays unreplayed.  Equal layouts go through the equal-rank forms."""
    from vidcom2_amd import _ffi
    F, N, D, dn, frames, params, cap = case
    C = params.channels(D) if params else D // 2
    assert tail_columns(C) > 0
    dev = torch.device("cuda:0")
    xd, ref, total, gidx, rows = _mode2_reference(F, N, D, dn, 2, params)
    if ref is not None:
        assert torch.equal(gidx.cpu(), ref["global_idx"])
    log = []
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        res, st = emulate_ranks(xd, list(frames), N, D, DTYPES[dn], 0.25, dev, params=params, vc_cap=cap or C,
                                spy=_spy_into(log))
    finally:
        _ffi.set_mode("torch")
    called = [n for n, _ in log]
    ragged = len(set(frames)) > 1
    sfx = "_ragged_o" if ragged else "_o"
    assert "vc2_video_centre_blocks" + sfx in called and "vc2_video_centre_finish_round" + sfx in called
    assert not any(("_ragged" in n) != ragged for n in called if n.startswith("vc2_video_centre_b"))
    if cap:
        assert called.count("vc2_video_centre_blocks_round" + sfx) == len(frames) * ((C + cap - 1) // cap - 1)
    # the tail records went through the exchange: the wide layout's stride, tail_records = 1 in the options
    assert all(s.vc_tail and s.blocks.shape[1] == 2 * 256 + 1 + max(frames) * N // 16 and s._opts.tail_records == 1 for s in st)
    print(case, "fragile", [s.vc_fragile for s in st], "max |d total|",
          float((torch.cat([s.total for s in st]) - total).abs().max()))
    assert all(s.vc_fragile == 0 for s in st)
    assert torch.equal(torch.cat([s.total for s in st]), total)
    assert torch.equal(torch.cat([r.global_idx for r in res]), gidx)
    assert torch.equal(torch.cat([r.rows for r in res]), rows)


@pytest.mark.gpu
def test_tail_chains_of_half_a_million_rows(_modes):
    """2688 x 196 x 72 bf16 split (1000, 1688): R = 526 848 > 2^19, so the plain columns cascade at level power 5 while the
    chains of R / 4 of the four tail columns (C = 36) stay at 4 -- two block sizes in one exchange.  Debug mode 2, against
    the unsharded pass in the same mode and the oracle."""
    from vidcom2_amd import _ffi
    F, N, D, frames = 2688, 196, 72, [1000, 1688]
    assert F * N > 1 << 19 and tail_record_plan([f * N for f in frames])[1] == 64
    dev = torch.device("cuda:0")
    xd, ref, total, gidx, rows = _mode2_reference(F, N, D, "bf16", 1, None)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        res, st = emulate_ranks(xd, frames, N, D, torch.bfloat16, 0.25, dev)
    finally:
        _ffi.set_mode("torch")
    assert all(s.vc_tail and s.vc_fragile == 0 for s in st)
    assert torch.equal(torch.cat([s.total for s in st]), total)
    assert torch.cat([r.ks for r in res]).cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(torch.cat([r.global_idx for r in res]), gidx)


@pytest.mark.gpu
def test_default_params_and_own_dtype_are_the_plain_pass(_modes):
    """params=PassParams() and score_dtype=x.dtype issue the plain constructor's entry points with its arguments."""
    F, N, D, frames = 8, 49, 64, [3, 5]
    dev = torch.device("cuda:0")
    xd = synth.make(F, N, D, torch.bfloat16, 2, "drift").to(dev)
    log_a, log_b = [], []
    res_a, st_a = emulate_ranks(xd, frames, N, D, torch.bfloat16, 0.25, dev, spy=_spy_into(log_a))
    res_b, st_b = emulate_ranks(xd, frames, N, D, torch.bfloat16, 0.25, dev, params=PassParams(),
                                score_dtype=torch.bfloat16, spy=_spy_into(log_b))
    assert all(s._opts is None for s in st_a + st_b)
    assert [n for n, _ in log_a] == [n for n, _ in log_b] and not any(n.endswith("_o") for n, _ in log_a)

    def plain(args):                # sizes and flags as they are; of a pointer (the two runs' buffers differ) whether it is given
        return [a if isinstance(a, (int, float)) else bool(a.value) if isinstance(a, ctypes.c_void_p) else a is not None
                for a in args]
    assert [plain(a) for _, a in log_a] == [plain(a) for _, a in log_b]
    assert torch.equal(torch.cat([s.total for s in st_a]), torch.cat([s.total for s in st_b]))
    assert torch.equal(torch.cat([r.global_idx for r in res_a]), torch.cat([r.global_idx for r in res_b]))
    assert torch.equal(torch.cat([r.rows for r in res_a]), torch.cat([r.rows for r in res_b]))


# ---- GPU, fp32 scoring ---------------------------------------------------------------------------------------------------

F32_CASES = [((16, 169, 512, "bf16", "drift", 0, None), (8, 8)), ((16, 169, 512, "bf16", "drift", 0, None), (5, 11)),
             ((16, 169, 512, "f16", "drift", 0, None), (8, 8)), ((16, 169, 512, "f16", "drift", 0, None), (5, 11)),
             ((8, 196, 1024, "bf16", "drift", 1, None), (3, 5)),
             ((5, 33, 256, "f16", "drift", 0, 0.75), (2, 3)),           # ratio 0.75, one scale
             ((4, 49, 64, "bf16", "drift", 0, 0.25), (1, 3))]           # ratio 0.25 (C = 16), temp 0.05, four scales
_WHOLE32 = {}


def _sd_case(F, N, D, dn, dist, seed, ratio):
    (c,) = [c for c in SD.load() if (c["F"], c["N"], c["D"], c["dtype"], c["dist"], c["seed"], c["ratio"], c["mapper"],
                                      c["base"]) == (F, N, D, dn, dist, seed, ratio, "linear", 0.25)]
    return c


def _whole32(key, c, xd):
    if key not in _WHOLE32:
        if len(_WHOLE32) > 1:
            _WHOLE32.clear()
        w = vc.compress(xd, c["N"], c["base"], want_scores=True, score_dtype=torch.float32,
                        params=params_of(c) if SD.has_params(c) else None)
        _WHOLE32[key] = ((w.v_score + w.f_score).float().flatten().clone(), w.ks.clone(), w.global_idx.clone(), w.rows.clone())
    return _WHOLE32[key]


@pytest.mark.gpu
@pytest.mark.parametrize("key,frames", F32_CASES,
                         ids=lambda a: "+".join(map(str, a)) if len(a) < 4 else "x".join(map(str, a[:3])) + f"-{a[3]}-r{a[6]}")
def test_sharded_pass_scores_16_bit_rows_in_fp32(key, frames, _modes):
    """score_dtype=torch.float32 over bf16 / fp16 shards, warnings as errors: budgets, kept indices and K are the
    reference's recorded ones (its pass over x.float(); decisions at least 5e-6 apart) and the unsharded fp32-scored pass's;
    the kept rows come in the storage dtype, bit for bit; the scores lie within two score tolerances plus one fp32 ulp of
    the largest total of the unsharded v + f; no video-centre record is exchanged."""
    c = _sd_case(*key)
    dt = DTYPES[c["dtype"]]
    x = SD.make_input(c)
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    dev = torch.device("cuda:0")
    xd = x.to(dev)
    total, ks, gidx, rows = _whole32(key, c, xd)
    params = params_of(c) if SD.has_params(c) else None
    log = []
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res, st = emulate_ranks(xd, list(frames), c["N"], c["D"], dt, c["base"], dev, params=params,
                                score_dtype=torch.float32, spy=_spy_into(log))
    got_total = torch.cat([s.total for s in st])
    got_ks, got_idx = torch.cat([r.ks for r in res]), torch.cat([r.global_idx for r in res])
    got_rows = torch.cat([r.rows for r in res])
    tol = 2 * SD.SCORE_TOL + float(np.spacing(np.float32(total.abs().max().item())))
    err = float((got_total - total).abs().max())
    print(key, frames, "ks", got_ks.tolist(), "reference", c["ks"], "max |d total|", err, "tol", tol)
    assert not any(n.startswith("vc2_video_centre_") for n, _ in log), {n for n, _ in log}
    assert all(s._opts is not None and s._opts.score_dtype == 0 and s.vc_fragile == 0 for s in st)
    assert got_ks.cpu().tolist() == c["ks"] and got_idx.cpu().tolist() == c["global_idx"] and sum(r.K for r in res) == c["K"]
    assert torch.equal(got_ks, ks) and torch.equal(got_idx, gidx)
    assert got_rows.dtype == dt and torch.equal(got_rows, rows) and torch.equal(got_rows.cpu(), x[got_idx.cpu()])
    assert got_total.dtype == torch.float32 and err <= tol


def _plain_sharded_pass_is_correct():
    x = make_input(8, 49, 64, "bf16", 2, "drift")
    dev = torch.device("cuda:0")
    O.set_mode("torch")
    ref = O.compress_indices(x, 49, 0.25)
    res, _ = emulate_ranks(x.to(dev), [3, 5], 49, 64, torch.bfloat16, 0.25, dev)
    assert torch.equal(torch.cat([r.global_idx for r in res]).cpu(), ref["global_idx"])


@pytest.mark.gpu
def test_limits_raise_at_construction(_modes):
    dev = torch.device("cuda:0")
    with pytest.raises(NotImplementedError):                # 8192 scored channels
        HipStages(2, 16, 8192, torch.bfloat16, dev, 0.25, params=PassParams(1.0))
    with pytest.raises(ValueError):                         # int(64 / 128) == 0 channels
        HipStages(2, 16, 64, torch.bfloat16, dev, 0.25, params=PassParams(1 / 128))
    with pytest.raises(NotImplementedError):
        ShardedCompressor(2, 16, 8192, torch.bfloat16, dev, 0.25, params=PassParams(1.0))
    with pytest.raises(ValueError):
        ShardedCompressor(2, 16, 64, torch.bfloat16, dev, 0.25, params=PassParams(1 / 128))
    with pytest.raises(ValueError):                         # fp16 scoring of bf16 rows does not exist
        ShardedCompressor(2, 16, 64, torch.bfloat16, dev, 0.25, score_dtype=torch.float16)
    with pytest.raises(ValueError):
        HipStages(2, 16, 64, torch.bfloat16, dev, 0.25, score_dtype=torch.float16)
    _plain_sharded_pass_is_correct()


@pytest.mark.gpu
@pytest.mark.parametrize("channels,temp,alphas,n,rc", [
    (0, 0.01, [1.0], None, -1), (513, 0.01, [1.0], None, -1), (-3, 0.01, [1.0], None, -1),
    (256, 0.0, [1.0], None, -1), (256, -1.0, [1.0], None, -1), (256, float("nan"), [1.0], None, -1),
    (256, float("inf"), [1.0], None, -1), (256, 0.01, [1.0, 0.0], None, -1), (256, 0.01, [-1.0], None, -1),
    (256, 0.01, [float("inf")], None, -1), (256, 0.01, [], 0, -1), (256, 0.01, [1.0] * 16, 17, -3)])
def test_c_abi_forms_refuse_bad_params_and_enqueue_nothing(channels, temp, alphas, n, rc, _modes):
    """The `_o` forms give vc2_compress_ex3's error codes for its bad sets; the buffers of a finished pass stay as they are."""
    from vidcom2_amd import _ffi, vidcom2 as V
    from vidcom2_amd.sharded import _CShardOpts
    from vidcom2_amd._ffi import ptr
    F, N, D = 4, 64, 512
    dev = torch.device("cuda:0")
    x = make_input(F, N, D, "bf16", 950, "drift").to(dev)
    st = HipStages(F, N, D, torch.bfloat16, dev, 0.25)
    stats = st.chan_stats(x).clone()
    st.select_channels(stats.reshape(-1, 2, D), F * N)
    csum = st.phase1(x).clone()
    s = st.phase2(x, csum.unsqueeze(0), F * N).clone()
    st.select(x, s, 0)
    torch.cuda.synchronize()
    keep = [t.clone() for t in (st.stats, st.csum, st.total, st.s, st.idx, st.ks, st.kout)]
    cp = V._CPassParams(channels, temp, len(alphas) if n is None else n,
                        (ctypes.c_double * 16)(*(list(alphas) + [1.0] * (16 - len(alphas)))))
    opts = _CShardOpts(ctypes.addressof(cp), st.code, 0)
    o, L, p, sp = ctypes.byref(opts), st._L, st._p, _ffi.stream_ptr(dev)
    C = csum.shape[1]                                       # (a valid channel count, so that only the params are refused)
    got = [L.vc2_chan_stats_o(ptr(x), F, N, D, st.code, F, st.bf, p["ws"], st._ws_n, p["stats"], sp, o),
           L.vc2_scores_phase1_o(ptr(x), F, N, D, st.code, p["cols"], C, p["spos"], p["perm"], p["var_f32"], F, p["ws"],
                                 st._ws_n, p["_csum_raw"], sp, o),
           L.vc2_scores_phase2_blocks_o(ptr(x), F, N, D, st.code, p["cols"], C, p["spos"], ptr(csum), csum.shape[0],
                                        csum.shape[1], csum.shape[0], F * N, p["ws"], st._ws_n, None, None, p["total"],
                                        p["s"], None, 0, st.vc_cap, sp, o),
           L.vc2_select_sharded_o(p["total"], ptr(s), F, 0, F, N, D, 0.25, st.code, p["ws"], st._ws_n, p["ks"], p["idx"],
                                  st.cap, p["kout"], ptr(x), p["rows"], sp, o)]
    assert got == [rc] * 4, (got, _ffi.last_error())
    bad_sd = _CShardOpts(None, 2, 0)                        # fp16 scoring of bf16 rows
    assert L.vc2_select_sharded_o(p["total"], ptr(s), F, 0, F, N, D, 0.25, st.code, p["ws"], st._ws_n, p["ks"], p["idx"],
                                  st.cap, p["kout"], ptr(x), p["rows"], sp, ctypes.byref(bad_sd)) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(keep, (st.stats, st.csum, st.total, st.s, st.idx, st.ks, st.kout)))


@pytest.mark.gpu
def test_real_collective_with_params_and_unequal_shards(_modes):
    """Two processes share cuda:0 over gloo, 5 and 3 frames of 8 x 49 x 64 bf16, ratio 0.75 (C = 48: sixteen tail columns),
    temp 0.05, four scales: ShardedCompressor, the HIP stages, a real padded collective.  Each child runs under its own time
    limit; nothing is started after a failure."""
    import tempfile
    frames = (5, 3)
    port = _free_port()
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    with tempfile.TemporaryDirectory() as tmp:
        outs = [os.path.join(tmp, f"rank{r}.pt") for r in range(2)]
        procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "_sharded_params.py"),
                                   str(r), ",".join(map(str, frames)), str(port), outs[r]], env=env, cwd=ROOT,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
        logs = [p.communicate()[0] for p in procs]                      # (the ranks need each other: started together)
        codes = [p.returncode for p in procs]
        assert codes == [0, 0], (codes, [lg[-2000:] for lg in logs])
        got = [torch.load(o) for o in outs]
    x = synth.make(8, 49, 64, torch.bfloat16, 2, "drift")
    whole = vc.compress(x.to("cuda:0"), 49, 0.25, params=GPU_CHILD_PARAMS)
    assert torch.equal(torch.cat([g["gidx"] for g in got]), whole.global_idx.cpu())
    assert torch.equal(torch.cat([g["ks"] for g in got]), whole.ks.cpu())
    assert torch.equal(torch.cat([g["rows"] for g in got]), whole.rows.cpu())
    assert all(torch.equal(g["all"], whole.global_idx.cpu()) for g in got)
    assert [g["fragile"] for g in got] == [0, 0]

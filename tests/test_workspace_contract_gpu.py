"""The two promises every entry point makes about its caller-owned workspace (include/vc2.h, vc2_workspace_bytes):

1. the bytes found in the workspace do not matter (sweep-1 partials under VC2_FLAG_HAVE_STATS excepted), and
2. a pass writes only inside [ws, ws + vc2_workspace_bytes) and inside the outputs' stated extents.

Every case runs once per pattern of tests/_guarded_ws.py -- `zero` (the baseline), `leftover` (another clip's finished
debug-mode pass), `ff`, `one` -- in an exactly sized workspace and exactly sized outputs between guard bands, the outputs'
interiors poisoned too.  Required: K, the status word, ks, the kept indices, the kept rows and both score tensors are
bit-identical to the `zero` run (NaN = NaN); status 0; every guard intact; vc2_selftest_counters unchanged.  The `zero`
run of a 16-bit `torch`-mode case is itself pinned to the CPU oracle where the oracle states the same pass (default
hyper-parameters through compress_indices, ratio / temp through the stage chain; not the 16-alpha case, which the oracle's
chain does not take, and not the chunked splits, which are no multiples of 16 frames and so promise the unsharded bits only
up to fp64 rounding of the exchanged sums).

fp32 arithmetic (fp32 inputs; score_dtype=torch.float32): the `zero` pattern is run twice first.  The two runs have been
bit-identical on every case (fixed-order fp64 reductions), and then bit-identity across patterns is demanded as for
16-bit; should they ever differ, the test falls back to exact ks / kept indices and scores within FP32_TOL.

The shapes are the smallest that take each route (DESIGN.md "Workspace regions: who writes before whom" is the map for a
failure here).  DESIGN.md also says why the chunked driver's `_csum_all` / `_blocks_all` stay `torch.zeros`: they are the
only shared buffers this module does not poison.
"""
import ctypes

import pytest
import torch

import _guarded_ws as G
import _margin_inputs as MI
import _range_inputs as RI
import oracle as O
from _stage_chain import FP32_TOL, oracle_chain, same
from vidcom2_amd import PassParams, _ffi, fused, synth
from vidcom2_amd import vidcom2 as V
from vidcom2_amd._ffi import DTYPE_CODE, lib, ptr, stream_ptr
from vidcom2_amd.chunked import ChunkedCompressor
from vidcom2_amd.vidcom2 import CompressPlan

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DN = {BF16: "bf16", F16: "f16", F32: "f32"}
MODES = {"torch": 4, "exact": 0, "torch_proven": 3, "debug2": 2}
OTHERS = [p for p in G.PATTERNS if p != "zero"]          # leftover first
BASE = 0.25


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _modes_back():
    yield
    assert lib().vc2_set_thread_mode(-1) == 0
    _ffi.set_mode("torch")
    O.set_mode("torch")
    G.clear_caches()


class Case:
    """One fused-pass case: shape, dtype, input, numerics mode, test seams (environment) and CompressPlan / enqueue options."""

    def __init__(self, name, F, N, D, dt, dist="drift", seed=9100, mode="torch", env=None, built=None, **kw):
        self.name, self.F, self.N, self.D, self.dt, self.dist, self.seed = name, F, N, D, dt, dist, seed
        self.mode, self.env, self.built, self.kw = mode, dict(env or {}), built, kw
        assert (F, N, D, dt) in G.SHAPES or kw.get("pool"), name
        self.id = f"{name}-{F}x{N}x{D}-{DN[dt]}-{dist}-{mode}" + "".join(f"-{k}{v}" for k, v in self.env.items())

    def input(self):
        if self.built is not None:
            return RI.build(self.built)
        return synth.make(self.F, self.N, self.D, self.dt, self.seed, self.dist)

    @property
    def fp32_arith(self):
        return self.dt == F32 or self.kw.get("score_dtype") == F32


def _cases():
    out = []
    # the one-launch variance + selection (k_var_select), its two-launch form and the LDS-round selection
    for dt in (BF16, F16):
        for mode in MODES:
            out.append(Case("varsel", 4, 49, 256, dt, mode=mode))
        out.append(Case("varsel", 4, 49, 256, dt, env={"VC2_VARSEL": "0"}))
        out.append(Case("varsel", 4, 49, 256, dt, env={"VC2_SEL4": "0"}))
    # the ORD form of sweep 2 (3x17x1024: N / 16 + 1 with a one-row tail block), and the same shapes without it
    for F, N in ((6, 196), (3, 17)):
        for dt in (BF16, F16):
            for dist in ("drift", "cancel"):
                out.append(Case("ord", F, N, 1024, dt, dist))
            out.append(Case("ord", F, N, 1024, dt, "cancel", env={"VC2_S2_ORD": "0"}))
    # ... on rows built against the norm replay margin (every planted row is queued and corrected)
    for c in MI.design_cases():
        if c["name"] in ("P1024-f16", "P3584-bf16"):
            out.append(Case("margin-" + c["name"], c["F"], c["N"], c["D"], RI.DT[c["dtype"]], built=c))
            out.append(Case("margin-" + c["name"], c["F"], c["N"], c["D"], RI.DT[c["dtype"]], built=c, env={"VC2_S2_ORD": "0"}))
    out.append(Case("scalar", 5, 50, 100, F16))
    out.append(Case("R<D", 1, 8, 512, BF16))
    out.append(Case("N=1", 16, 1, 64, BF16))
    out.append(Case("N=1", 16, 1, 64, F16))
    out.append(Case("fp32", 3, 50, 96, F32))
    out.append(Case("wide", 2, 33, 4104, BF16))
    out.append(Case("scalesF", 1024, 4, 64, BF16))
    out.append(Case("scalesF", 1025, 4, 64, BF16))
    # options at 4x49x256 bf16
    o = lambda name, **kw: out.append(Case(name, 4, 49, 256, BF16, **kw))
    o("noscores", want_scores=False)
    o("tail2", tail_rows=2)
    o("mirror", mirror=True)
    o("grid-img", grid="img")
    o("grid-newline", grid="newline")
    o("nogather", gather=False)
    o("C=D", params=PassParams(1.0))
    o("C=1", params=PassParams(1 / 256))
    o("C=37", params=PassParams(37 / 256))
    o("temp", params=PassParams(0.5, 0.05))
    o("alphas16", params=PassParams(0.5, 0.01, [0.05 * (i + 1) for i in range(16)]))
    o("score32", score_dtype=F32)
    o("score32-C=37", score_dtype=F32, params=PassParams(37 / 256))
    # pool_stats, then the pass on its partials (VC2_FLAG_HAVE_STATS): the pattern is applied BEFORE pool_stats -- the
    # partials are its output, everything else in the buffer stays poisoned
    for pm in ("average", "bilinear"):
        out.append(Case("pool-" + pm, 2, 49, 256, BF16, pool=pm))
    return out


CASES = _cases()
assert len({c.id for c in CASES}) == len(CASES)
_baseline = {}           # case id -> the zero run(s), computed once and never changed


def _set_mode(mode):
    assert lib().vc2_set_mode(MODES[mode]) == 0


def _cpu(t):
    return None if t is None else t.detach().cpu().clone()


def _run(c, pattern, monkeypatch):
    """One pass of case `c` in guarded, patterned workspace and outputs: the outputs on the host, checked for status 0,
    intact guards and unchanged self-test counters."""
    d, F, N, D, kw = dev(), c.F, c.N, c.D, c.kw
    with monkeypatch.context() as mp:
        for k, v in c.env.items():
            mp.setenv(k, v)
        _set_mode(c.mode)
        x = c.input().to(d)
        x0 = x.clone()
        grid = kw.get("grid")
        h = int(round(N ** 0.5)) if grid else 0
        img = synth.make(F, h * (h + 1), D, c.dt, c.seed + 5000, c.dist).to(d) if grid == "img" else None
        nl = synth.make(1, 1, D, c.dt, c.seed + 6000, "iid").reshape(D).to(d) if grid == "newline" else None
        tail_rows = kw.get("tail_rows", 0)
        tail = synth.make(1, tail_rows, D, c.dt, c.seed + 7000, "iid").to(d) if tail_rows else None
        with G.patched_workspace(mp, pattern) as rec:
            before = G.selftest_counters()
            ws, flat = None, x
            if kw.get("pool"):
                xin = synth.make(F, 196, D, c.dt, c.seed, c.dist).view(F, 196, D).to(d)
                pooled, ws = fused.pool_stats(xin, 14, 14, kw["pool"])
                flat = x = pooled.view(F * N, D)
                x0 = x.clone()
            plan = CompressPlan(F, N, D, c.dt, d, BASE, "grid_vid" if grid else "linear", h, kw.get("want_scores", True),
                                kw.get("gather", True), tail_rows, ws=ws, score_dtype=kw.get("score_dtype"),
                                params=kw.get("params"))
            assert len(rec.guards) == 1, "the plan (or pool_stats) took its workspace through _ffi.workspace"
            out, ogs = G.guarded_outputs(plan, pattern)
            plan.out = out                                   # (finish() reads the plan's own set: the mirrored case)
            plan.enqueue(flat, gather_src=img, tail=tail, have_stats=ws is not None, mirror=kw.get("mirror", False),
                         out=out, newline=nl)
            if kw.get("mirror"):
                early = plan.finish()                        # returns on the pinned mirror's early words
                plan._settle()                               # ... and the final status word (raises on a late guard hit)
            torch.cuda.synchronize()
            K, status = (int(w) for w in out.kout.tolist())
            if kw.get("mirror"):
                assert early.K == K
            assert status == 0, f"status word {status:#x}"
            assert 0 < K <= plan.cap
            assert rec.intact(), rec.damage()
            for name, g in zip([n for n in OutputSet_fields(out)], ogs):
                assert g.intact(), f"output {name}: {g.damage()}"
            assert G.selftest_counters() == before, "a selection guard fired"
            assert torch.equal(x, x0), "the input was modified"
            got = dict(K=K, status=status, ks=_cpu(out.ks), idx=_cpu(out.idx[:K]),
                       rows=None if out.rows is None else _cpu(out.rows[:K + tail_rows]), v=_cpu(out.v), f=_cpu(out.f))
            src = img if grid == "img" else x
            if grid == "newline":
                src = torch.cat([x.view(F, h, h, D), nl.expand(F, h, 1, D)], 2).reshape(-1, D)
            got["x"], got["src"], got["tail"] = _cpu(x), _cpu(src), _cpu(tail)
    return got


def OutputSet_fields(out):
    return [n for n in out._fields if getattr(out, n) is not None]


def _identical(a, b):
    ok = a["K"] == b["K"] and a["status"] == b["status"] and torch.equal(a["ks"], b["ks"]) and torch.equal(a["idx"], b["idx"])
    for k in ("rows", "v", "f"):
        ok = ok and ((a[k] is None) == (b[k] is None)) and (a[k] is None or same(a[k], b[k]))
    return ok


def _what_differs(a, b):
    out = [k for k in ("K", "status") if a[k] != b[k]]
    out += [k for k in ("ks", "idx") if a[k].shape != b[k].shape or not torch.equal(a[k], b[k])]
    out += [k for k in ("rows", "v", "f") if a[k] is not None and not same(a[k], b[k])]
    return out


def _check_structure(c, g):
    """What holds for every pass whatever the oracle says: K is the budgets' sum, the rows are the gathered-from tensor's."""
    F, N, kw = c.F, c.N, c.kw
    h = int(round(N ** 0.5)) if kw.get("grid") else 0
    assert g["K"] == int(g["ks"].clamp(max=N).sum()) + F * h
    assert bool((g["idx"] >= 0).all()) and bool((g["idx"] < g["src"].shape[0]).all())
    if g["rows"] is not None:
        want = g["src"][g["idx"]]
        if g["tail"] is not None:
            want = torch.cat([want, g["tail"]])
        assert same(g["rows"], want), "rows != src[idx] (+ tail)"


def _check_oracle(c, g):
    """The zero run of a 16-bit `torch`-mode case against the CPU oracle."""
    kw = c.kw
    if c.mode != "torch" or c.fp32_arith:
        return
    p = kw.get("params")
    if p is not None and tuple(p.alphas) != (0.125, 0.25, 0.5, 1.0, 2.0):
        return                                               # (the oracle's chain takes ratio and temp, not the scales)
    O.set_mode("torch")
    x, F, N = g["x"], c.F, c.N
    if p is None:
        ref = O.compress_indices(x, N, BASE)
        ks, keep, v, f = ref["ks"], ref["global_idx"], ref["v"], ref["f"]
    else:
        ch = oracle_chain(x, N, BASE, p.channel_ratio, p.temp)
        ks, keep, v, f = torch.tensor(ch["ks"]), ch["keep"], ch["v"], ch["f"]
    assert g["ks"].tolist() == ks.tolist(), "budgets != oracle"
    if kw.get("grid"):
        h = int(round(N ** 0.5))
        loc = keep - torch.repeat_interleave(torch.arange(F) * N, ks)
        keep = O.map_grid_vid(list(torch.split(loc, ks.tolist())), h)
    assert torch.equal(g["idx"], keep), "kept indices != oracle"
    if g["v"] is not None:
        assert same(g["v"], v) and same(g["f"], f), "scores != oracle"


def baseline(c, monkeypatch):
    if c.id not in _baseline:
        runs = [_run(c, "zero", monkeypatch)]
        if c.fp32_arith:
            runs.append(_run(c, "zero", monkeypatch))
        _baseline[c.id] = runs
    return _baseline[c.id]


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_zero_workspace_is_the_pinned_baseline(c, monkeypatch):
    runs = baseline(c, monkeypatch)
    _check_structure(c, runs[0])
    _check_oracle(c, runs[0])
    if c.fp32_arith:
        print(c.id, "two zero runs bit-identical:", _identical(runs[0], runs[1]), _what_differs(runs[0], runs[1]))
        assert runs[0]["K"] == runs[1]["K"] and torch.equal(runs[0]["ks"], runs[1]["ks"]) \
            and torch.equal(runs[0]["idx"], runs[1]["idx"])


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("pattern", OTHERS)
def test_workspace_contents_do_not_matter(pattern, c, monkeypatch):
    runs = baseline(c, monkeypatch)
    got = _run(c, pattern, monkeypatch)
    if not c.fp32_arith or _identical(runs[0], runs[1]):
        assert _identical(got, runs[0]), f"{pattern}: {_what_differs(got, runs[0])} differ from the zero run"
        return
    # fp32 arithmetic whose own repeat is not bit-identical: the kept set exactly, the scores within FP32_TOL
    assert got["K"] == runs[0]["K"] and torch.equal(got["ks"], runs[0]["ks"]) and torch.equal(got["idx"], runs[0]["idx"])
    for k in ("v", "f"):
        if got[k] is not None:
            err = float((got[k].double() - runs[0][k].double()).abs().max())
            print(c.id, pattern, k, "max |d|", err, "bound", FP32_TOL)
            assert err <= FP32_TOL


# ---- the stage wrappers ---------------------------------------------------------------------------------------------
def _stage_run(pattern, monkeypatch, dt=BF16):
    """_channel_variance, select_low_var_channels, compute_gaussian_scores (workspaces through the patch), compute_scales
    and _select (their own small scratch: the same C calls with a guarded, patterned scratch of the wrappers' size)."""
    d, F, N, D = dev(), 4, 49, 256
    _set_mode("torch")
    x = synth.make(F, N, D, dt, 9200, "drift").to(d)
    code, L = DTYPE_CODE[dt], lib()
    with G.patched_workspace(monkeypatch, pattern) as rec:
        before = G.selftest_counters()
        var_T, var_f = V._channel_variance(x)
        sel = V.select_low_var_channels(x)
        v, f = V.compute_gaussian_scores(sel, N)
        assert len(rec.guards) == 3                          # (1, R, D) twice -- the variance -- and (F, N, C)
        s = -v.mean(dim=-1)
        total = v + f
        extra = []

        def gt(shape, tdt):
            t, g = G.guarded_tensor(shape, tdt, d, pattern)
            extra.append(g)
            return t
        scales = gt((F,), dt)
        ws1, g1 = G.guarded(3 * (F * 4 + 256), pattern, d)
        assert L.vc2_compute_scales(ptr(s), F, BASE, 0.01, code, ptr(ws1), ws1.numel(), ptr(scales), stream_ptr(d)) == 0
        ws2, g2 = G.guarded(F * N * 4 + F * 4 + 1024, pattern, d)
        ks, offs, idx, kout = gt((F,), torch.int64), gt((F + 1,), torch.int64), gt((F * N,), torch.int64), gt((2,), torch.int64)
        assert L.vc2_select(ptr(total), ptr(scales), F, N, N, code, _ffi.MAP_LINEAR, 0, ptr(ws2), ws2.numel(), ptr(ks),
                            ptr(offs), ptr(idx), F * N, ptr(kout), stream_ptr(d)) == 0
        torch.cuda.synchronize()
        K, status = (int(w) for w in kout.tolist())
        assert status == 0 and 0 < K <= F * N
        assert rec.intact(), rec.damage()
        for g in extra + [g1, g2]:
            assert g.intact(), g.damage()
        assert G.selftest_counters() == before
        return dict(x=_cpu(x), var_T=_cpu(var_T), var_f=_cpu(var_f), sel=_cpu(sel), v=_cpu(v), f=_cpu(f), scales=_cpu(scales),
                    ks=_cpu(ks), offs=_cpu(offs), idx=_cpu(idx[:K]), K=K)


_stage_base = {}


def _stage_baseline(monkeypatch, dt):
    if dt not in _stage_base:
        _stage_base[dt] = _stage_run("zero", monkeypatch, dt)
    return _stage_base[dt]


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_stage_wrappers_zero_run_equals_the_oracle_chain(dt, monkeypatch):
    g = _stage_baseline(monkeypatch, dt)
    O.set_mode("torch")
    ch = oracle_chain(g["x"], 49, BASE)
    assert same(g["sel"], ch["sel"]) and same(g["v"], ch["v"]) and same(g["f"], ch["f"]) and same(g["scales"], ch["scales"])
    assert g["ks"].tolist() == ch["ks"] and torch.equal(g["idx"], ch["keep"])
    assert same(g["var_T"], O.chan_var(g["x"]))


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("pattern", OTHERS)
def test_stage_wrappers_ignore_workspace_contents(pattern, dt, monkeypatch):
    base = _stage_baseline(monkeypatch, dt)
    got = _stage_run(pattern, monkeypatch, dt)
    bad = [k for k in base if k != "K" and not same(got[k], base[k])]
    assert got["K"] == base["K"] and not bad, f"{pattern}: {bad} differ from the zero run"


# ---- frame-sharded stages without a process group: the chunked driver -----------------------------------------------
CHUNKED = [("7-2-7", (7, 2, 7), 49, 256, BF16, "torch"), ("5-1-1-5", (5, 1, 1, 5), 5, 128, F16, "debug2")]


def _chunked_run(cc, pattern, monkeypatch):
    name, frames, N, D, dt, mode = cc
    d = dev()
    _set_mode(mode)
    x = synth.make(sum(frames), N, D, dt, 9400, "cancel" if mode == "debug2" else "drift").to(d)
    chunks = [t.clone() for t in torch.split(x, [f * N for f in frames])]
    with G.patched_workspace(monkeypatch, pattern) as rec:
        before = G.selftest_counters()
        comp = ChunkedCompressor(list(frames), N, D, dt, d, BASE)
        assert len(rec.guards) == len(frames)                # one HipStages workspace per chunk
        # the shared `torch.empty` buffers, poisoned right after construction; _csum_all / _blocks_all are documented
        # torch.zeros and stay zero (their padding rows / unused record cells are read and never written)
        st0 = comp.stages[0]
        for t in (comp._stats_all, comp._s_all, comp._total, st0.var_f32, st0.mask, st0.cols, st0.perm, st0.spos, comp._sel_ws):
            G.fill(t.view(-1).view(torch.uint8), pattern)
        res = comp(chunks)
        torch.cuda.synchronize()
        assert rec.intact(), rec.damage()
        assert G.selftest_counters() == before
        assert same(res.rows, x[res.global_idx])
        return dict(K=res.K, ks=_cpu(res.ks), idx=_cpu(res.global_idx), rows=_cpu(res.rows))


_chunk_base = {}


@pytest.mark.parametrize("cc", CHUNKED, ids=lambda cc: cc[0])
@pytest.mark.parametrize("pattern", OTHERS)
def test_chunked_stages_ignore_workspace_contents(pattern, cc, monkeypatch):
    if cc[0] not in _chunk_base:
        _chunk_base[cc[0]] = _chunked_run(cc, "zero", monkeypatch)
    base = _chunk_base[cc[0]]
    got = _chunked_run(cc, pattern, monkeypatch)
    bad = [k for k in ("ks", "idx", "rows") if got[k].shape != base[k].shape or not same(got[k], base[k])]
    assert got["K"] == base["K"] and not bad, f"{pattern}: {bad} differ from the zero run"


# ---- a workspace one byte short: VC2_ERR_WORKSPACE, nothing enqueued, the next call works ----------------------------
ERR_WORKSPACE = -5


def _short_route(route, monkeypatch):
    """Per route: (call(ws_bytes) -> rc, [output tensors], F, N, D, dtype of the workspace)."""
    d, dt = dev(), BF16
    F, N, D = 4, 49, 256
    code, st = DTYPE_CODE[dt], stream_ptr(dev())
    x = synth.make(F, N, D, dt, 9500, "drift").to(d)
    outs, gs = [], []

    def gt(shape, tdt):
        t, g = G.guarded_tensor(shape, tdt, d, "ff")
        outs.append(t)
        gs.append(g)
        return t
    L = lib()
    if route == "compress":
        cap = int(L.vc2_kept_capacity(F, N, BASE))
        rows, idx, ks, kout, v, f = gt((cap, D), dt), gt((cap,), torch.int64), gt((F,), torch.int64), gt((2,), torch.int64), \
            gt((F, N), dt), gt((F, N), dt)
        shape = (F, N, D)
        call = lambda ws, n: L.vc2_compress_ex5(ptr(x), F, N, D, code, BASE, 0, 0, ptr(x), F * N, ptr(ws), n, ptr(rows),
                                                ptr(idx), cap, ptr(ks), ptr(kout), ptr(v), ptr(f), None, 0, 0, None, None,
                                                code, None, st)
    elif route == "chan_var":
        var_T, var_f = gt((D,), dt), gt((D,), F32)
        shape = (1, F * N, D)
        call = lambda ws, n: L.vc2_chan_var(ptr(x), F * N, D, code, ptr(ws), n, ptr(var_T), ptr(var_f), st)
    elif route == "scores":
        v, f = gt((F, N), dt), gt((F, N), dt)
        shape = (F, N, D)
        call = lambda ws, n: L.vc2_scores(ptr(x), F, N, D, code, None, D, None, ptr(ws), n, ptr(v), ptr(f), None, None, st)
    elif route == "pool_stats":
        xin = synth.make(F, 196, D, dt, 9501, "drift").view(F, 196, D).to(d)
        pooled = gt((F, 49, D), dt)
        shape = (F, 49, D)
        call = lambda ws, n: L.vc2_pool_stats(ptr(xin), F, 14, 14, D, code, 1, ptr(ws), n, ptr(pooled), st)
    else:
        bst = gt((F, 2, D), torch.float64)
        shape = (F, N, D)
        call = lambda ws, n: L.vc2_chan_stats(ptr(x), F, N, D, code, F, 1, ptr(ws), n, ptr(bst), st)
    return call, outs, gs, shape, dt


@pytest.mark.parametrize("route", ["compress", "chan_var", "scores", "pool_stats", "chan_stats"])
def test_workspace_one_byte_short_is_refused_and_enqueues_nothing(route, monkeypatch):
    _set_mode("torch")
    call, outs, gs, shape, dt = _short_route(route, monkeypatch)
    ws, g = G.guarded(_ffi.workspace_bytes(*shape, dt), "one", dev())
    snap = [t.clone() for t in outs]
    assert call(ws, ws.numel() - 1) == ERR_WORKSPACE, _ffi.last_error()
    torch.cuda.synchronize()
    assert g.intact() and all(x.intact() for x in gs)
    assert bool((ws == 0x01).all()), "the refused call wrote into the workspace"
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, snap)), "the refused call wrote an output"
    assert call(ws, ws.numel()) == 0, _ffi.last_error()       # the next, correct call works
    torch.cuda.synchronize()
    assert g.intact(), g.damage()
    assert all(x.intact() for x in gs)
    assert not all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(outs, snap))


# ---- one workspace size per shape ------------------------------------------------------------------------------------
def test_workspace_sized_in_exact_mode_serves_a_torch_pass(monkeypatch):
    """6x196x1024 bf16 takes the ORD form in `torch` mode, whose block sums (o_bsum) `exact` mode does not use: a caller
    that sized its workspace in `exact` and then switched got VC2_ERR_WORKSPACE."""
    F, N, D, dt, d = 6, 196, 1024, BF16, dev()
    _ffi.set_mode("exact")
    ws, g = G.guarded(_ffi.workspace_bytes(F, N, D, dt), "ff", d)
    _ffi.set_mode("torch")
    x = synth.make(F, N, D, dt, 9100, "drift")
    plan = CompressPlan(F, N, D, dt, d, BASE, want_scores=True, ws=ws)
    out, ogs = G.guarded_outputs(plan, "ff")
    plan.out = out
    plan.enqueue(x.to(d), out=out)
    res = plan.finish()
    torch.cuda.synchronize()
    assert g.intact(), g.damage()
    assert all(o.intact() for o in ogs)
    ref = O.compress_indices(x, N, BASE)
    assert res.ks.cpu().tolist() == ref["ks"].tolist() and torch.equal(res.global_idx.cpu(), ref["global_idx"])
    assert same(res.v_score, ref["v"]) and same(res.f_score, ref["f"])

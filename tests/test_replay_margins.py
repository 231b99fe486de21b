"""The replay margins of the token norm and the squared-distance sums, on rows built against them.

In the `torch` modes a 16-bit pass computes both sums exactly and replays torch's own fp32 order only where the exact
value lies within a margin of fp32-ulps of a T rounding boundary.  Every other fixture is `iid` / `drift` / `cancel` data
or a magnitude edit: torch's chains err by ~10 ulps there, with random signs, and a margin of 16 would pass them all.
tests/_margin_inputs.py plants rows on which every rounding of torch's norm chain errs the same way (tens to a thousand
ulps; tests/golden/margin_cases.json, make_margin_golden.py: the reference's own results and, per case, `needs_ulps`, the
margin a pass must use to give the reference's norm for every row).

a. host arithmetic (no GPU): vc2_selftest_margins against bounds derived here from the oracle's summation structure
b. CPU: the oracle's two accumulation orders, driven with absorption patterns, against exact sums
c. family S (compute_gaussian_scores on a tensor taken as selected) and family P (the whole pass, one case with a
   channel ratio of its own, and two logical ranks)
   against the reference's digests in `torch`, `torch_proven` and debug mode 2; `exact` mode against the oracle's
d. which cases may be skipped (SKIP RULE below), and that the in-margin ones are not

The bounds (a.).  A sum of non-negative fp32 terms whose deepest path has k roundings, each of relative error <= 2^-24:
|torch's sum - exact| <= k 2^-24 exact (first order).  Distance sums are rounded as they are, and v 2^-24 < ulp(v): within
k ulps, k + 1 with the rounding of RN_f32(exact) that the pass holds.  Norms: the correctly rounded square root halves
the relative error, k / 2 ulps, + 1 for the two final roundings.  k by walking the oracle's loops (norm_torch_order:
bf16 2 (C / 16) + 7 + C % 16 >= ceil(C / 8) + 7, fp16 C; sum_torch_order: _cascade_depth).

SKIP RULE.  No case is skipped in `torch_proven`, debug mode 2 or `exact`, and no bf16 case in `torch`.  An fp16 case
is skipped in `torch` only when its recorded needs_ulps exceeds the norm margin vc2_selftest_margins reports for
(C, fp16, mode 4) -- and 120, whatever that margin is: the default keeps the empirical 128 ulps for fp16 (DESIGN.md section 3 has the measurement) and
returns the exactly rounded norm for such rows.  test_skip_rule counts them."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _margin_inputs as MI
import _range_inputs as RI
import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd._ffi import check, lib

from conftest import load_json

CASES = load_json("margin_cases.json")["cases"]
S_CASES = [c for c in CASES if c["family"] == "S"]
P_CASES = [c for c in CASES if c["family"] == "P"]
DT_CODE = {"f32": 0, "bf16": 1, "f16": 2}
MODES = ["torch", "torch_proven", "replay_all"]
IN_MARGIN = 120          # needs_ulps up to here: a case every margin so far must get right -- never skipped
MODE_CODE = {"exact": 0, "torch_fast": 1, "replay_all": 2, "torch_proven": 3, "torch": 4}


def cid(c):
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}"


scored_channels = MI.scored_channels


def _params(c):
    return None if c["ratio"] is None else vc.PassParams(channel_ratio=c["ratio"])


def margins(C, dn, mode):
    out = (ctypes.c_int32 * 2)()
    check(lib().vc2_selftest_margins(C, DT_CODE[dn], MODE_CODE[mode], out), "vc2_selftest_margins")
    return out[0], out[1]


def may_skip(c, mode):
    """The SKIP RULE of the module docstring."""
    return mode == "torch" and c["dtype"] == "f16" and c["needs_ulps"] > max(margins(scored_channels(c), "f16", "torch")[0], IN_MARGIN)


# ---- a. the margins against bounds derived from the oracle's summation structure ---------------------------------------
def _norm_depth(C, dn):
    """Roundings along the deepest path of oracle/vc2_oracle.cpp norm_torch_order (every fused multiply-add and add
    counted, also the first into a zero accumulator)."""
    if dn == "f16":
        return C                                        # one sequential chain
    nv = C // 16 * 16                                   # whole vectors: element p to chain p % 8
    d = nv // 8                                         # ... C / 8 fused multiply-adds per chain
    for _ in range(1, 8):
        d = max(d, nv // 8) + 1                         # s = acc[0]; s += acc[j]
    return d + (C - nv)                                 # the tail, one after the other


def _cascade_depth(C):
    """The same for sum_torch_order (16-bit types: chunks of 16, 8 lanes x 4 interleaved vectors, 4 levels), walking its
    loops with d(a + b) = max(d(a), d(b)) + 1.  The 8 lanes are alike; the 4 interleaved vectors are tracked apart."""
    vec_size = C // 16
    size_ilp = vec_size // 4
    lp = max(4, (size_ilp - 1).bit_length() // 4 if size_ilp > 1 else 0)
    step, mask = 1 << lp, (1 << lp) - 1
    acc = [[None] * 4 for _ in range(4)]                # [level][ilp]: None = still an exact zero

    def add(a, b):
        return b if a is None else a if b is None else max(a, b) + 1

    i = 0
    while i + step <= size_ilp:
        for _ in range(step):
            for k in range(4):
                acc[0][k] = add(acc[0][k], 1) if acc[0][k] is not None else 1      # load: p[j] + p[8 + j], one rounding
            i += 1
        for j in range(1, 4):
            for k in range(4):
                acc[j][k] = add(acc[j][k], acc[j - 1][k])
                acc[j - 1][k] = None
            if i & (mask << (j * lp)):
                break
    while i < size_ilp:
        for k in range(4):
            acc[0][k] = add(acc[0][k], 1) if acc[0][k] is not None else 1
        i += 1
    for j in range(1, 4):
        for k in range(4):
            acc[0][k] = add(acc[0][k], acc[j][k])
    for _ in range(size_ilp * 4, vec_size):
        acc[0][0] = add(acc[0][0], 1) if acc[0][0] is not None else 1
    for k in range(1, 4):
        acc[0][0] = add(acc[0][0], acc[0][k])
    lane = acc[0][0]
    fin = C - vec_size * 16 or None                     # the C % 16 tail, one after the other (fin = 0; fin += v)
    for _ in range(8):
        fin = add(fin, lane)
    return fin or 0


def test_cascade_depth_walk_matches_hand_counts():
    """C = 4096: one rounding in the load, 15 adds at level 0, 3 level-1 adds (a first add into an empty accumulator is
    exact), the upper levels empty, 3 vectors, 7 lanes."""
    assert _cascade_depth(4096) == 1 + 15 + 3 + 0 + 3 + 7
    assert _norm_depth(1792, "bf16") == 224 + 7 and _norm_depth(4096, "bf16") == 519 and _norm_depth(1001, "bf16") == 124 + 7 + 9
    assert all(_norm_depth(C, "bf16") >= -(-C // 8) + 7 for C in range(64, 4097))


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_margins_are_bounds(dn):
    """Host arithmetic only.  Norm margin: >= k / 2 + 1 in `torch_proven` and debug mode 2 for both 16-bit types, and in
    every torch-order mode for bf16; distance margin: >= k + 1 in every torch-order mode; nothing is replayed in `exact`
    mode or for fp32.  Every C from 64 to 4096."""
    depth_of_vecs = {}
    for C in range(64, 4097):
        norm_bound = (_norm_depth(C, dn) + 1) // 2 + 1
        key = (C // 16, C % 16)
        if key not in depth_of_vecs:
            depth_of_vecs[key] = _cascade_depth(C)
        dist_bound = depth_of_vecs[key] + 1
        for mode in ("torch", "torch_fast", "torch_proven", "replay_all"):
            nm, dm = margins(C, dn, mode)
            if dn == "bf16" or mode in ("torch_proven", "replay_all"):
                assert nm >= norm_bound, (C, dn, mode, nm, norm_bound)
            assert nm >= 128                            # the margin of every earlier fixture still holds
            assert dm >= dist_bound, (C, dn, mode, dm, dist_bound)
            assert max(nm, dm) + 64 < 1 << (15 if dn == "bf16" else 12)       # (+ the sweeps' own allowance) inside half a T interval
        assert margins(C, dn, "exact") == (-1, -1)
    assert margins(1792, "f32", "torch") == (-1, -1)
    # what the bounds come to (documented in vc2_kernels.hip, include/vc2.h and DESIGN.md section 3)
    assert margins(1792, "bf16", "torch") == (128, 48) and margins(4096, "bf16", "torch")[0] == 261
    if dn == "f16":
        assert margins(1792, "f16", "torch_proven")[0] == 897 and margins(4096, "f16", "replay_all")[0] == 2049
    out = (ctypes.c_int32 * 2)()
    assert lib().vc2_selftest_margins(0, 1, 4, out) < 0 and lib().vc2_selftest_margins(64, 1, 5, out) < 0
    assert lib().vc2_selftest_margins(64, 1, 4, None) < 0


# ---- b. the oracle's two orders against exact sums, on absorption patterns ---------------------------------------------
def _ulp32(v):
    return 2.0 ** (math.floor(math.log2(v)) - 23)


def _rnT(v32, dt):
    return float(torch.tensor(v32, dtype=torch.float32).to(dt))


def _boundary_distance(v32, dn):
    return int(MI.needs_ulps(torch.tensor([v32], dtype=torch.float64), dn)[0])


def _absorbing_rows(C, dt, rng, trials):
    """Rows of non-negative T values for the cascade: in chain (vector k, lane l) every level-0 block starts with a head
    and goes on with values whose pair sums stay below half an ulp of it, so every add of the block is absorbed; heads
    and block structure vary from trial to trial, and some chains get a large head in their first block only, so that
    the level-1 adds are absorbed as well."""
    nb = 8 if dt == torch.bfloat16 else 11
    for t in range(trials):
        row = np.zeros(C)
        head = (1 + rng.integers(0, 1 << (nb - 1)) / (1 << (nb - 1))) * 2.0 ** int(rng.integers(6, 12))
        tiny = 2.0 ** (math.floor(math.log2(head)) - 26) * (1 + rng.integers(0, 1 << (nb - 1)) / (1 << nb))   # 2 tiny < ulp / 2
        period = [16, 16, 8, 32][t % 4]                 # loads per head: the cascade's block, or off it
        big_first = t % 3 == 0
        for p in range(C // 16 * 16):
            c, j = divmod(p, 16)
            i = c // 4
            row[p] = head if (j < 8 and i % period == 0) else tiny
            if big_first and j < 8 and i == 0:
                row[p] = head * 2.0 ** (20 if dt == torch.bfloat16 else 3)
        row[C // 16 * 16:] = tiny
        yield torch.tensor(row, dtype=torch.float64).to(dt)


@pytest.mark.parametrize("C", [1792, 4096])
@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_distance_margin_on_absorption_patterns(C, dn):
    """torch's cascade order (oracle.sum_torch_order) against the exact sum: the error stays inside the bound derived in
    a. and so inside the distance margin, and wherever the two round to different T values the exact sum is within the
    margin of the boundary."""
    dt = RI.DT[dn]
    rng = np.random.default_rng(C + len(dn))
    bound, margin = _cascade_depth(C) + 1, margins(C, dn, "torch")[1]
    assert bound <= margin
    worst = 0.0
    for row in _absorbing_rows(C, dt, rng, 240):
        exact = float(row.double().sum())
        e32 = float(np.float32(exact))
        got = O.sum_torch_order(row, dt)
        err = abs(got - exact) / _ulp32(exact)
        worst = max(worst, err)
        assert err <= bound, (err, bound)
        if _rnT(got, dt) != _rnT(e32, dt):
            assert _boundary_distance(e32, dn) <= margin
    assert worst >= 6.0, worst                          # the patterns do make the cascade err one way


@pytest.mark.parametrize("c", S_CASES, ids=cid)
def test_norm_order_on_planted_rows(c):
    """CPU: on a planted row the oracle's norm order errs by what the fixture records (needs_ulps is the distance of the
    exact norm from the boundary that torch's value is on the other side of), inside the bound of a."""
    x = RI.build(c)
    row = x[RI.mixed_rows(c["F"], c["N"])[0]]
    dt = RI.DT[c["dtype"]]
    exact = float(row.double().norm())
    got = O.norm_torch_order(row, dt)
    err = abs(got - exact) / _ulp32(exact)
    assert c["needs_ulps"] <= err + 1 <= (_norm_depth(c["D"], c["dtype"]) + 1) // 2 + 2, (err, c["needs_ulps"])
    assert _rnT(got, dt) != _rnT(float(np.float32(exact)), dt)


# ---- d. the skip rule -----------------------------------------------------------------------------------------------
def test_skip_rule():
    """Counts: nothing but fp16 cases in `torch` mode is ever skipped, each of them needs more than the margin the default
    mode has, and every in-margin case (needs_ulps <= 120) of both dtypes runs in every mode; each dtype has at least
    two in-margin cases above 32 ulps and two above 200."""
    skipped = [(c["name"], m) for c in CASES for m in MODES + ["exact"] if may_skip(c, m)]
    assert all(m == "torch" and n.endswith("-f16") for n, m in skipped)
    by = {c["name"]: c for c in CASES}
    for n, _ in skipped:
        assert by[n]["needs_ulps"] > 128
    # with the default's empirical fp16 margin of 128: the four S and three P cases whose chains are longer than 512
    assert sorted(n for n, _ in skipped) == sorted(c["name"] for c in CASES if c["dtype"] == "f16" and scored_channels(c) > 512)
    assert len(skipped) == 7 and len(CASES) * 4 - len(skipped) == 69
    for dn in ("bf16", "f16"):
        need = [c["needs_ulps"] for c in CASES if c["dtype"] == dn]
        inside = [c for c in CASES if c["dtype"] == dn and 32 < c["needs_ulps"] <= IN_MARGIN]
        assert len(inside) >= 2 and sum(n > 200 for n in need) >= 2, (dn, need)
        assert not any(may_skip(c, m) for c in inside for m in MODES + ["exact"])
    for c in CASES:                                     # the premises the generator asserted
        assert c["norm_ne"] >= c["planted"] and (c["v_sha256"] != c["exact_v_sha256"] or c["f_sha256"] != c["exact_f_sha256"])
        assert c["oracle_torch_mode"]["scores"] is True


# ---- c. on the GPU ----------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _default_mode():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")
    if torch.cuda.is_available():
        out = (ctypes.c_int32 * 8)()                    # no loop bound of the selection replay expired
        check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
        assert list(out) == [0] * 8, list(out)


def dev():
    return torch.device("cuda:0")


_INPUTS = {}


def _input(c):
    if c["name"] not in _INPUTS:
        x = RI.build(c)
        assert synth.sha256_tensor(x) == c["x_sha256"]
        _INPUTS[c["name"]] = x
    return _INPUTS[c["name"]]


def _set(mode):
    if mode == "replay_all":
        assert lib().vc2_set_mode(2) == 0
    else:
        _ffi.set_mode(mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", S_CASES, ids=cid)
def test_stage_route(c, mode):
    """compute_gaussian_scores on the tensor as selected (vc2_scores, cols = NULL): the reference's v and f."""
    if may_skip(c, mode):
        pytest.skip(f"fp16 default mode: needs {c['needs_ulps']} ulps, the empirical margin is "
                    f"{margins(scored_channels(c), 'f16', 'torch')[0]}")
    xd = _input(c).to(dev())
    keep = xd.clone()
    _set(mode)
    v, f = vc.compute_gaussian_scores(xd, c["N"])
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.uint8), keep.view(torch.uint8)), "input was modified"
    assert RI.score_sha256(v) == c["v_sha256"], ("v", mode)
    assert RI.score_sha256(f) == c["f_sha256"], ("f", mode)


@pytest.mark.gpu
@pytest.mark.parametrize("c", S_CASES, ids=cid)
def test_stage_route_exact_mode(c):
    x = _input(c)
    _ffi.set_mode("exact")
    O.set_mode("exact")
    v, f = vc.compute_gaussian_scores(x.to(dev()), c["N"])
    ov, of = O.compute_gaussian_scores(x, c["N"])
    assert RI.score_sha256(ov) == c["exact_v_sha256"] and RI.score_sha256(of) == c["exact_f_sha256"]
    assert RI.score_sha256(v) == c["exact_v_sha256"], "v"
    assert RI.score_sha256(f) == c["exact_f_sha256"], "f"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", P_CASES, ids=cid)
def test_whole_pass(c, mode):
    """vc.compress: the reference's budgets, kept indices, rows and score digests (test_value_range's contract)."""
    from test_value_range import _check_vs_golden
    if may_skip(c, mode):
        pytest.skip(f"fp16 default mode: needs {c['needs_ulps']} ulps, the empirical margin is "
                    f"{margins(scored_channels(c), 'f16', 'torch')[0]}")
    xd = _input(c).to(dev())
    keep = xd.clone()
    _set(mode)
    got = vc.compress(xd, c["N"], c["base"], want_scores=True, params=_params(c))
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.uint8), keep.view(torch.uint8)), "input was modified"
    _check_vs_golden(got, c, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("c", P_CASES, ids=cid)
def test_whole_pass_exact_mode(c):
    from test_value_range import _check_vs_oracle
    x = _input(c)
    _ffi.set_mode("exact")
    O.set_mode("exact")
    got = vc.compress(x.to(dev()), c["N"], c["base"], want_scores=True, params=_params(c))
    torch.cuda.synchronize()
    if c["ratio"] is None:
        ref = O.compress_indices(x, c["N"], c["base"])
    else:                                               # (the oracle's whole-pass entry has no ratio: its stage chain)
        from _stage_chain import oracle_chain
        o = oracle_chain(x, c["N"], c["base"], c["ratio"])
        ref = dict(ks=torch.tensor(o["ks"]), global_idx=o["keep"], v=o["v"], f=o["f"])
    assert RI.score_sha256(ref["v"]) == c["exact_v_sha256"] and RI.score_sha256(ref["f"]) == c["exact_f_sha256"]
    _check_vs_oracle(got, ref, x, c["dtype"], "exact")


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [("P3584-bf16", "torch"), ("P2048-f16", "torch_proven")])
def test_two_logical_ranks(name, mode):
    """vc2_scores_phase1 carries the same margins: two logical ranks (test_sharded's emulation on one GPU) give the
    unsharded pass's scores and the reference's budgets, kept indices and rows."""
    from test_sharded import _emulate_ranks_on_one_gpu
    from test_value_range import _check_vs_golden
    c = next(c for c in P_CASES if c["name"] == name)
    assert not may_skip(c, mode)
    xd = _input(c).to(dev())
    _set(mode)
    whole = vc.compress(xd, c["N"], c["base"], want_scores=True)
    _check_vs_golden(whole, c, "unsharded")
    res, st = _emulate_ranks_on_one_gpu(xd, c["F"], c["N"], c["D"], RI.DT[c["dtype"]], c["base"], 2, dev())
    assert torch.equal(torch.cat([s.total for s in st]), (whole.v_score + whole.f_score).float().flatten())
    ks = torch.cat([r.ks for r in res]).cpu()
    gidx = torch.cat([r.global_idx for r in res]).cpu()
    assert ks.tolist() == c["ks"] and synth.sha256_tensor(gidx) == c["idx_sha256"]
    assert torch.equal(torch.cat([r.rows for r in res]), whole.rows)

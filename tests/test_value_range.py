"""Extreme feature magnitudes against the reference's vectors (tests/golden/range_cases.json, make_range_golden.py) and
the CPU oracle.  Every other fixture keeps every row inside the windows of sweep 2's fast paths; these inputs
(tests/_range_inputs.py) leave them -- at D % 8 != 0 (VEC = 1) and through the grid mapper too: rows go to the exact path of k_norm_colsum2 / k_norm_colsum (fp64 sum of squares,
exact division, rflag = 1 for sweep 3), into the ORD block chains and the fp64 frame sums from there, and -- where
torch's fp32 sum of squares overflows (norm inf, x^ = +-0) -- to k_norm_fix's torch-order replay.

The contract is test_long_frames.py's: budgets, kept indices and rows the reference's, half-precision scores bit for
bit in the `torch` and `torch_proven` modes and in debug mode 2 (every norm, distance and mean replayed); `exact` mode
equals the oracle's `exact` mode.  fp32 scores are compared with the oracle's `torch` mode within 1e-6 (its norm takes
torch's fp32 overflow; the pass does the same for fp32 rows whose sum of squares rounds to inf in fp32)."""
import ctypes

import numpy as np
import pytest
import torch

import _range_inputs as RI
import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd._ffi import check, lib

from conftest import load_json
from test_long_frames import _with_env

pytestmark = pytest.mark.gpu
RANGE = load_json("range_cases.json")
CASES = RANGE["cases"]


@pytest.fixture(autouse=True)
def _default_mode():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")
    out = (ctypes.c_int32 * 8)()                                  # no loop bound of the selection replay expired
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)


def dev():
    return torch.device("cuda:0")


def cid(c):
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}"


def _input(c):
    x = RI.build(c)
    assert synth.sha256_tensor(x) == c["x_sha256"]
    return x


def _check_vs_golden(got, c, what=""):
    """test_long_frames._check_vs_golden with NaN scores compared as NaN (RI.score_sha256)."""
    gi = got.global_idx.cpu()
    assert got.ks.cpu().tolist() == c["ks"], ("budgets", what)
    assert got.K == c["K"] and synth.sha256_tensor(gi) == c["idx_sha256"], ("kept indices", what)
    assert synth.sha256_tensor(got.rows) == c["out_sha256"], ("rows", what)
    if c["dtype"] == "f32":
        assert np.allclose(got.v_score[0, :16].cpu().tolist(), c["v_head"], rtol=0, atol=1e-5, equal_nan=True), ("v", what)
        assert np.allclose(got.f_score[0, :16].cpu().tolist(), c["f_head"], rtol=0, atol=1e-5, equal_nan=True), ("f", what)
    else:
        assert RI.score_sha256(got.v_score) == c["v_sha256"], ("v_score", what)
        assert RI.score_sha256(got.f_score) == c["f_sha256"], ("f_score", what)


def _max_diff(a, b):
    """max |a - b| with NaN against NaN as 0 (NaN against a number stays NaN: the comparison fails)."""
    a, b = a.double().cpu(), b.double().cpu()
    d = (a - b).abs()
    return torch.where(a.isnan() & b.isnan(), torch.zeros_like(d), d).max().item()


def _check_vs_oracle(got, ref, x, dn, what=""):
    """test_long_frames._check_vs_oracle with NaN scores equal to NaN and kept rows compared bitwise (they may hold
    NaN)."""
    gi = got.global_idx.cpu()
    assert got.ks.cpu().tolist() == ref["ks"].tolist(), ("budgets", what)
    assert got.K == int(ref["global_idx"].numel()) and torch.equal(gi, ref["global_idx"]), ("kept indices", what)
    assert torch.equal(got.rows.cpu().view(torch.uint8), x[gi].view(torch.uint8)), ("rows", what)
    if dn == "f32":
        assert _max_diff(got.v_score, ref["v"]) <= 1e-6 and _max_diff(got.f_score, ref["f"]) <= 1e-6, ("scores", what)
    else:
        assert RI.score_sha256(got.v_score) == RI.score_sha256(ref["v"]), ("v_score", what)
        assert RI.score_sha256(got.f_score) == RI.score_sha256(ref["f"]), ("f_score", what)


def _check(got, c, x, what):
    _check_vs_golden(got, c, what)
    if c["dtype"] == "f32":
        O.set_mode("torch")
        _check_vs_oracle(got, O.compress_indices(x, c["N"], c["base"]), x, "f32", what)


# ---- a. the reference's own vectors, in every mode that claims them --------------------------------------------------
@pytest.mark.parametrize("mode", ["torch", "torch_proven", "replay_all"])
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_range_cases(c, mode):
    x = _input(c)
    xd = x.to(dev())
    keep = xd.clone()
    if mode == "replay_all":
        assert lib().vc2_set_mode(2) == 0
    else:
        _ffi.set_mode(mode)
    got = vc.compress(xd, c["N"], c["base"], want_scores=True)
    torch.cuda.synchronize()
    assert torch.equal(xd.view(torch.uint8), keep.view(torch.uint8)), "input was modified"
    _check(got, c, x, mode)


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_range_cases_exact_mode(c):
    """`exact` mode: the oracle's `exact` mode (fp64 norms: no overflow, finite quotients)."""
    x = _input(c)
    _ffi.set_mode("exact")
    O.set_mode("exact")
    got = vc.compress(x.to(dev()), c["N"], c["base"], want_scores=True)
    torch.cuda.synchronize()
    _check_vs_oracle(got, O.compress_indices(x, c["N"], c["base"]), x, c["dtype"], "exact")


# ---- a2. LLaVA-Video's grid mapper -------------------------------------------------------------------------------------
GRID = [c for c in CASES if c.get("grid_h")]


@pytest.mark.parametrize("mode", ["torch", "replay_all"])
@pytest.mark.parametrize("c", GRID, ids=cid)
def test_grid_cases(c, mode):
    """mapper "grid_vid" (13 x 13 tokens per frame, img_feat of a 13 x 14 grid): the reference's budgets, mapped
    indices and gathered img_feat rows -- through the pass and through vidcom2_compression(model="llava_vid")."""
    x, img = _input(c), RI.grid_img(c)
    assert synth.sha256_tensor(img) == c["img_sha256"]
    if mode == "replay_all":
        assert lib().vc2_set_mode(2) == 0
    h = c["grid_h"]
    got = vc.compress(x.to(dev()), c["N"], c["base"], "grid_vid", h, img.to(dev()))
    torch.cuda.synchronize()
    assert got.ks.cpu().tolist() == c["ks"] and got.K == c["grid_K"]
    assert synth.sha256_tensor(got.global_idx) == c["grid_idx_sha256"]
    assert synth.sha256_tensor(got.rows) == c["grid_out_sha256"]
    out = vc.vidcom2_compression(x.to(dev()), model="llava_vid", base_scale=c["base"], img_feat=img.to(dev()))
    assert synth.sha256_tensor(out) == c["grid_out_sha256"]


# ---- b. both forms of sweep 2 ----------------------------------------------------------------------------------------
S2 = [c for c in CASES if c["dtype"] != "f32" and c["D"] in (1024, 3584, 4096) and c["N"] <= 512]


@pytest.mark.parametrize("ord_form", ["1", "0"])
@pytest.mark.parametrize("c", S2, ids=cid)
def test_both_sweep2_forms(c, ord_form):
    """VC2_S2_ORD = 1 (frame sums in torch's order inside sweep 2, the exact rows in the block chains) and 0 (margins
    and replays)."""
    x = _input(c)
    got = _with_env("VC2_S2_ORD", ord_form, lambda: vc.compress(x.to(dev()), c["N"], c["base"], want_scores=True))
    torch.cuda.synchronize()
    _check_vs_golden(got, c, f"VC2_S2_ORD={ord_form}")


# ---- c. the frame-sharded pass and a batch next to an ordinary clip --------------------------------------------------
SHARDED = [c for c in CASES if c["name"] in ("B3584-bf16-ovf", "C3584-f16-8x16384") and c["F"] == 8]


@pytest.mark.parametrize("P", [2, 4])
@pytest.mark.parametrize("c", SHARDED, ids=cid)
def test_frame_sharded(c, P):
    """P logical ranks (test_sharded's emulation on one GPU): the unsharded pass's scores, the reference's budgets,
    kept indices and rows."""
    from test_sharded import _emulate_ranks_on_one_gpu
    x = _input(c)
    xd = x.to(dev())
    whole = vc.compress(xd, c["N"], c["base"], want_scores=True)
    _check_vs_golden(whole, c, "unsharded")
    res, st = _emulate_ranks_on_one_gpu(xd, c["F"], c["N"], c["D"], RI.DT[c["dtype"]], c["base"], P, dev())
    assert torch.equal(torch.cat([s.total for s in st]), (whole.v_score + whole.f_score).float().flatten())
    ks = torch.cat([r.ks for r in res]).cpu()
    gidx = torch.cat([r.global_idx for r in res]).cpu()
    assert ks.tolist() == c["ks"] and synth.sha256_tensor(gidx) == c["idx_sha256"]
    assert torch.equal(torch.cat([r.rows for r in res]), whole.rows)


@pytest.mark.parametrize("c", SHARDED, ids=cid)
def test_batch_next_to_an_ordinary_clip(c):
    """compress_batch of the case and an ordinary clip of the same shape: the case gives the reference's result, the
    ordinary clip what it gives alone."""
    x = _input(c)
    plain = synth.make(c["F"], c["N"], c["D"], RI.DT[c["dtype"]], c["seed"], c["dist"]).to(dev())
    alone = vc.compress(plain, c["N"], c["base"])
    for order in ((x.to(dev()), plain), (plain, x.to(dev()))):
        got = vc.compress_batch(list(order), c["N"], c["base"])
        torch.cuda.synchronize()
        r_case, r_plain = (got[0], got[1]) if order[1] is plain else (got[1], got[0])
        assert r_case.ks.cpu().tolist() == c["ks"] and synth.sha256_tensor(r_case.global_idx.cpu()) == c["idx_sha256"]
        assert synth.sha256_tensor(r_case.rows) == c["out_sha256"]
        assert torch.equal(r_plain.ks, alone.ks) and torch.equal(r_plain.global_idx, alone.global_idx)
        assert torch.equal(r_plain.rows, alone.rows)


# ---- d. scale invariance across both window limits -------------------------------------------------------------------
@pytest.mark.parametrize("s", RANGE["sweeps"], ids=lambda s: s["name"])
def test_scale_invariance(s):
    """x 2^e for every e where the goldens show the reference unchanged: the same score bits and kept indices as the
    unscaled clip (the reference's), though the rows leave sweep 2's fast path below 2^-39 and above 2^40 (bf16)."""
    for e in s["invariant_e"]:
        got = vc.compress(RI.sweep_input(s, e).to(dev()), s["N"], s["base"], want_scores=True)
        torch.cuda.synchronize()
        assert RI.score_sha256(got.v_score) == s["v_sha256"], e
        assert RI.score_sha256(got.f_score) == s["f_sha256"], e
        assert synth.sha256_tensor(got.global_idx) == s["idx_sha256"], e

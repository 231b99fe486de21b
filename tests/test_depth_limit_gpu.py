"""GPU: the selection / sort replay (vidcom2_amd/csrc/vc2_select2.h) on inputs that drive libstdc++'s nth_element and sort
into their depth-limit fall-backs, with ties (tests/golden/make_depth_limit_golden.py): __heap_select + iter_swap after
2 floor(log2 n) partitions, heapsort of a segment at depth 0.  Those branches permute tied elements, so they decide the
kept set and the channel order; every fixture's answer is torch.topk's on the CPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi
from vidcom2_amd._ffi import check, lib, ptr, stream_ptr

from _depth_limit import DTYPES, TORCH_DT, load, pass_input, rank_values

pytestmark = pytest.mark.gpu
KAT = load()
BY = {c["name"]: c for c in KAT}
ENGINES = ({}, {"VC2_SEL4": "0"})
FORMS = ({}, {"VC2_VARSEL": "0"}, {"VC2_SEL4": "0"})
KEYS = ("VC2_SEL4", "VC2_VARSEL")


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _modes_and_guards():
    """Default numerics mode before and after; the fall-backs are libstdc++'s own path, not a guard: no counter moves."""
    _ffi.set_mode("torch")
    O.set_mode("torch")
    c = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(c, 1), "vc2_selftest_counters")          # (start from zero: read and reset)
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")
    torch.cuda.synchronize()
    check(lib().vc2_selftest_counters(c, 0), "vc2_selftest_counters")
    assert list(c) == [0] * 8, list(c)


class env:
    """Set the selection's test switches for a block; restore what was there."""
    def __init__(self, form):
        self.form = form

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KEYS}
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(self.form)

    def __exit__(self, *exc):
        for k in KEYS:
            os.environ.pop(k, None)
            if self.old[k] is not None:
                os.environ[k] = self.old[k]


def chan_select(t, k, order):
    """vc2_chan_select on fp32-widened values -> (mask | None, cols, perm, order, opos, spos)."""
    n = t.numel()
    mk = lambda dt=torch.int32: torch.full((n,), -1, dtype=dt, device=dev())       # noqa: E731
    cols = mk()
    if not order:
        mask = torch.zeros(n, dtype=torch.uint8, device=dev())
        check(lib().vc2_chan_select(ptr(t), n, k, ptr(mask), ptr(cols), None, None, None, None, stream_ptr(dev())), "chan_select")
        return mask, cols, None, None, None, None
    perm, order_, opos, spos = mk(), mk(), mk(), mk()
    check(lib().vc2_chan_select(ptr(t), n, k, None, ptr(cols), ptr(perm), ptr(order_), ptr(opos), ptr(spos), stream_ptr(dev())),
          "chan_select")
    return None, cols, perm, order_, opos, spos


@pytest.mark.parametrize("form", ENGINES, ids=lambda f: "sel4" if not f else "lds")
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("c", [c for c in KAT if c["kind"] == 0], ids=lambda c: c["name"])
def test_chan_select_set(c, dn, form):
    """The kept SET at the selection's depth limit: introselect4 (16-bit values, D <= 4096), the LDS rounds of introselect2
    (VC2_SEL4=0, D = 8192) and the 64-bit words of chan_select_body<uint64_t> (fp32 values)."""
    n, k = c["n"], c["k"]
    t = rank_values(c["ranks"], dn).float().to(dev())
    want = sorted(c["out"].tolist())
    with env(form):
        mask, cols, *_ = chan_select(t, k, False)
        torch.cuda.synchronize()
    assert mask.cpu().nonzero().flatten().tolist() == want
    assert cols[:k].cpu().tolist() == want and bool((cols[k:] == -1).all())


@pytest.mark.parametrize("form", ENGINES, ids=lambda f: "sel4" if not f else "lds")
@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("c", [c for c in KAT if c["kind"] != 0], ids=lambda c: c["name"])
def test_chan_select_order(c, dn, form):
    """torch.topk(sorted=True)'s ORDER where std::sort heap-sorts a segment at depth 0 (and, for the patterns built by the
    selection adversary, where nth_element met its limit first)."""
    n, k = c["n"], c["k"]
    t = rank_values(c["ranks"], dn).float().to(dev())
    want = c["out"].tolist()
    with env(form):
        _, cols, perm, order, opos, spos = chan_select(t, k, True)
        torch.cuda.synchronize()
    assert cols[:k].cpu().tolist() == sorted(want)
    assert sorted(perm[:k].cpu().tolist()) == sorted(want)
    assert order[:k].cpu().tolist() == want
    assert cols[opos[:k].long()].cpu().tolist() == want
    assert order[spos[:k].long()].cpu().tolist() == cols[:k].cpu().tolist()


FRAME_SHAPES = ("tail64", "solo196", "solo324", "lds729", "coop1024", "coop8192")


@pytest.mark.parametrize("dn", DTYPES)
@pytest.mark.parametrize("name", FRAME_SHAPES)
def test_per_frame_selection(name, dn):
    """k_select, every engine split of select_frame_body (N <= 256, <= 512, <= 1020, > 1020; 32-bit words for 16-bit scores,
    64-bit for fp32): killer, ordinary tie-heavy, killer, a different killer, ordinary -- each frame its own answer.  (A
    status word that is not 0 raises.)"""
    a, b = BY[name], BY[name + "b"]
    n = a["n"]
    ks = [a["k"], a["k"], a["k"], b["k"], b["k"]]                # (the second killer answers another budget)
    rng = np.random.RandomState(n)
    ordinary = [rank_values(rng.randint(0, 40, size=n), dn) for _ in range(2)]
    rows = [rank_values(a["ranks"], dn), ordinary[0], rank_values(a["ranks"], dn), rank_values(b["ranks"], dn), ordinary[1]]
    scores = torch.stack(rows).contiguous()
    scales = torch.tensor([k / n for k in ks], dtype=torch.float32).to(TORCH_DT[dn])
    assert O.compute_ks(scales, n) == ks
    want = [sorted(a["out"].tolist()), None, sorted(a["out"].tolist()), sorted(b["out"].tolist()), None]
    for i in (1, 4):
        want[i] = torch.topk(scores[i], ks[i], largest=False, sorted=False).indices.sort().values.tolist()
    got = vc.select_outlier_indices(scores.to(dev()), scales.to(dev()), n)
    for i in range(5):
        assert got[i].cpu().tolist() == want[i], f"frame {i}"


def test_no_fall_back_fixture_per_frame():
    """n = 40 ends on its last allowed partition without the fall-back (the certificate's "no"): one wave, the register tail."""
    c = BY["nofb40"]
    for dn in DTYPES:
        scores = rank_values(c["ranks"], dn).repeat(3, 1).contiguous()
        scales = torch.full((3,), c["k"] / c["n"], dtype=torch.float32).to(TORCH_DT[dn])
        got = vc.select_outlier_indices(scores.to(dev()), scales.to(dev()), c["n"])
        assert all(g.cpu().tolist() == sorted(c["out"].tolist()) for g in got)


def _nan_eq(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


@pytest.mark.parametrize("mode", ["torch", "torch_proven"])
@pytest.mark.parametrize("c", [c for c in KAT if c["kind"] == 2], ids=lambda c: c["name"])
def test_fused_pass(c, mode):
    """A real pass whose channel variances carry a killer pattern: k_var_select's polled selection and sweep 2's ORDER riders
    (the nparts > 1 walk of introsort2) meet the depth limits; channel order, budgets, kept indices and scores are the
    oracle's bit for bit in every launch form."""
    F, N = c["F"], c["N"]
    x = pass_input(c["ranks"], F, N, c["dtype"])
    ref = O.compress_indices(x, N, 0.25)
    xd = x.to(dev())
    _ffi.set_mode(mode)
    for form in FORMS:
        with env(form):
            r = vc.compress(xd, N, 0.25, want_scores=True)                 # (a status word that is not 0 raises)
            chan = vc.vidcom2.low_var_channel_order(xd)
            torch.cuda.synchronize()
        assert chan.cpu().tolist() == c["out"].tolist(), form
        assert r.ks.cpu().tolist() == ref["ks"].tolist(), form
        assert torch.equal(r.global_idx.cpu(), ref["global_idx"]), form
        assert _nan_eq(r.v_score, ref["v"]) and _nan_eq(r.f_score, ref["f"]), form


def test_fused_pass_scored_in_fp32():
    """score_dtype=float32: the variances are fp32 (amplitude^2 exactly: same order, same ties, not 16-bit representable), the
    selection takes the 64-bit words.  Channel order and kept indices are the reference's on the widened input."""
    c = BY["pass512s"]
    F, N = c["F"], c["N"]
    x = pass_input(c["ranks"], F, N, c["dtype"])
    ref = O.compress_indices(x.float(), N, 0.25)
    xd = x.to(dev())
    r = vc.compress(xd, N, 0.25, score_dtype=torch.float32)
    chan = vc.vidcom2.low_var_channel_order(xd.float())
    torch.cuda.synchronize()
    assert chan.cpu().tolist() == c["out"].tolist()
    assert r.ks.cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(r.global_idx.cpu(), ref["global_idx"])

"""CPU: the depth-limit fixtures (tests/golden/make_depth_limit_golden.py) still mean what their certificates say -- the
oracle's topk and live torch.topk give the recorded answers in every dtype, and the certificates are consistent."""
import numpy as np
import pytest
import torch

import oracle as O
from _depth_limit import DTYPES, load, pass_input, rank_values

KAT = load()
SEL2_ONE_WAVE = 1020          # sel2_capacity(1, 4): heap-sorted segments on both sides of it are asked for


@pytest.mark.parametrize("c", KAT, ids=lambda c: c["name"])
def test_oracle_and_live_torch_topk_give_the_recorded_answer(c):
    for dn in DTYPES:
        t = rank_values(c["ranks"], dn)
        assert t.isfinite().all() and (t > 0).all()
        assert len(torch.unique(t)) == len(np.unique(c["ranks"]))                  # the rule keeps order and ties
        assert (dn == "f32") == bool((t.float().view(torch.int32) & 0x1FFF).ne(0).any())   # 16-bit representable or not
        want = torch.from_numpy(c["out"])
        assert torch.equal(torch.topk(t, c["k"], largest=False, sorted=c["sorted"]).indices, want), dn
        assert torch.equal(O.topk_smallest(t, c["k"], c["sorted"]), want), dn


@pytest.mark.parametrize("c", [c for c in KAT if c["kind"] == 2], ids=lambda c: c["name"])
def test_pass_inputs_carry_the_rank_pattern_in_their_variances(c):
    x = pass_input(c["ranks"], c["F"], c["N"], c["dtype"])
    assert x.shape == (c["F"] * c["N"], c["n"])
    dense = np.unique(c["ranks"], return_inverse=True)[1]
    for var in (x.var(0, unbiased=False), x.float().var(0, unbiased=False)):
        assert np.array_equal(np.unique(var.float().numpy(), return_inverse=True)[1], dense)
        assert torch.equal(torch.topk(var, c["k"], largest=False).indices, torch.from_numpy(c["out"]))
    idx, _ = O.select_low_var_channel_idx(x, 0.5)
    assert torch.equal(idx, torch.from_numpy(c["out"]))


def test_certificates_are_consistent():
    by = {c["name"]: c for c in KAT}
    assert not by["nofb40"]["sel_hit"] and by["nofb40"]["sel_len"] == 0           # the certificate can say "no"
    for c in KAT:
        n, k, r = c["n"], c["k"], c["ranks"]
        assert r.size == n and c["out"].size == k and k * 64 > n
        kth = np.sort(r)[k - 1]
        group = np.flatnonzero(r == kth)
        kept = np.intersect1d(group, c["out"])
        assert (group.size, kept.size) == (c["group"], c["group_kept"])
        assert set(np.flatnonzero(r < kth).tolist()) <= set(c["out"].tolist())
        both = not np.array_equal(kept, group[:kept.size]) and not np.array_equal(kept, group[group.size - kept.size:])
        assert c["naive_differs"] == (0 < kept.size < group.size and both)
        if c["kind"] == 0:
            assert c["sel_hit"] == (c["name"] != "nofb40")
            if c["name"] + "b" in by:                              # the per-frame test's second killer: same shape, own budget
                assert by[c["name"] + "b"]["n"] == n and by[c["name"] + "b"]["k"] > k
            assert 0 < kept.size < group.size                      # the k-th value is tied across the boundary
            if not c["name"].endswith("b"):                        # (every engine's first killer; the second ones as they come)
                assert c["naive_differs"]                          # ... and neither naive tie rule gives the kept set
            if c["sel_hit"]:
                assert 3 < c["sel_len"] <= n and not c["segs"]
                assert c["sel_pops"] > 0 and c["flip_differs"]     # the fall-back decides the set, down to the heap's tie step
        elif c["kind"] == 1 or c["name"].endswith("o"):
            assert c["sorted"] and c["segs"] and any(c["seg_dup"]) and c["disorder"]
            for (f, l), dup in zip(c["segs"], c["seg_dup"]):
                assert 0 <= f and l <= k - 1 and l - f > 16
                v = r[c["out"][f:l]]
                assert (np.diff(v.astype(np.int64)) >= 0).all() and dup == bool((np.diff(v.astype(np.int64)) == 0).any())
        else:                                                      # pass*s: the polled selection of the pass meets its limit
            assert c["sel_hit"] and c["sel_pops"] > 0 and c["naive_differs"]
    lens = [l - f for c in KAT if c["kind"] == 1 for (f, l) in c["segs"]]
    assert min(lens) < SEL2_ONE_WAVE < max(lens)
    assert sorted(c["k"] - 1 for c in KAT if c["kind"] == 1) == [100, 400, 1791, 4095, 5999]

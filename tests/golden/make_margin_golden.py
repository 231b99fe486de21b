#!/usr/bin/env python
"""Replay-margin goldens from the REFERENCE (build container only: needs the reference checkout).

    python tests/golden/make_margin_golden.py      ->  tests/golden/margin_cases.json

Inputs whose planted rows make torch's fp32 norm accumulation err in one direction, by tens to hundreds of fp32-ulps
(tests/_margin_inputs.py).  Family S: the reference's compute_gaussian_scores on an [F * N, C] tensor as it is; family P:
the whole pass.  Stored as digests in range_cases.json's layout (budgets in full), plus the premises, asserted here -- a
case without them is not written:
    norm_ne      rows whose reference norm differs from RN_T of the fp64 norm: at least the planted rows
    needs_ulps   over those rows, the largest distance (fp32-ulps) from RN_f32 of the exact norm to its T rounding
                 boundary: the replay margin a pass needs to give the reference's norm for every row
    the reference's v / f digests differ from those of the oracle's `exact` mode (stored as exact_*_sha256; v_ne / f_ne:
                 how many scores of each differ -- at least one of the two digests must)
and, per dtype, at least two cases with needs_ulps in (32, 120] and at least two above 200.
Nothing of the reference's source is copied.
"""
from __future__ import annotations

import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")

from token_compressor.vidcom2 import vidcom2 as R  # noqa: E402  (the reference)

import _margin_inputs as MI  # noqa: E402
import _range_inputs as RI  # noqa: E402
import oracle as O  # noqa: E402
from _stage_chain import hook_chain, oracle_chain  # noqa: E402
from make_range_golden import reference, vs_oracle  # noqa: E402
from vidcom2_amd import synth  # noqa: E402

torch.set_grad_enabled(False)


def premises(c, sel, ref_norm, rv, rf, ev, ef):
    exact64 = sel.double().norm(dim=-1)
    ne = ref_norm.double() != exact64.to(sel.dtype).double()
    need = int(MI.needs_ulps(exact64, c["dtype"])[ne].max()) if bool(ne.any()) else 0
    p = dict(norm_ne=int(ne.sum()), needs_ulps=need)
    assert p["norm_ne"] >= c["planted"], (c["name"], p)
    p.update(v_ne=int((rv != ev).sum()), f_ne=int((rf != ef).sum()))          # scores that move with the norms
    assert RI.score_sha256(rv) != RI.score_sha256(ev) or RI.score_sha256(rf) != RI.score_sha256(ef), c["name"]
    return p


def record(c, x):
    N = c["N"]
    if c["family"] == "S":
        v, f = R.compute_gaussian_scores(x, N)
        O.set_mode("exact")
        ev, ef = O.compute_gaussian_scores(x, N)
        O.set_mode("torch")
        tv, tf = O.compute_gaussian_scores(x, N)
        O.set_mode("exact")
        rec = dict(c, x_sha256=synth.sha256_tensor(x), v_sha256=RI.score_sha256(v), f_sha256=RI.score_sha256(f),
                   exact_v_sha256=RI.score_sha256(ev), exact_f_sha256=RI.score_sha256(ef),
                   oracle_torch_mode=dict(scores=bool(torch.equal(tv, v) and torch.equal(tf, f))))
        rec.update(premises(c, x, x.norm(2, -1), v, f, ev, ef))
        return rec
    if c["ratio"] is not None:
        return record_ratio(c, x)
    r = reference(x, N, c["base"])
    g, chan = r["g"], RI.low_var_channels(x)
    O.set_mode("exact")
    oe = O.compress_indices(x, N, c["base"])
    O.set_mode("torch")
    ot = O.compress_indices(x, N, c["base"])
    O.set_mode("exact")
    rec = dict(c, x_sha256=synth.sha256_tensor(x), ks=r["ks"], K=int(g.numel()), idx_sha256=synth.sha256_tensor(g),
               idx_head=g[:8].tolist(), idx_tail=g[-8:].tolist(), v_sha256=RI.score_sha256(r["v"]),
               f_sha256=RI.score_sha256(r["f"]), chan_sha256=synth.sha256_tensor(chan), out_sha256=synth.sha256_tensor(x[g]),
               exact_v_sha256=RI.score_sha256(oe["v"]), exact_f_sha256=RI.score_sha256(oe["f"]),
               oracle_torch_mode=vs_oracle(ot, r, x, chan), oracle_exact_mode=vs_oracle(oe, r, x, chan))
    assert torch.equal(oe["chan_idx"], chan), c["name"]
    rec.update(premises(c, x[:, chan], r["norm"], r["v"], r["f"], oe["v"], oe["f"]))
    return rec


def record_ratio(c, x):
    """A P case with a channel ratio of its own: the reference's stage chain with that ratio (the oracle's whole-pass
    entry has no such argument: its stage chain, tests/_stage_chain.py)."""
    N = c["N"]
    r = hook_chain(R, x, N, c["base"], c["ratio"])
    O.set_mode("exact")
    oe = oracle_chain(x, N, c["base"], c["ratio"])
    O.set_mode("torch")
    ot = oracle_chain(x, N, c["base"], c["ratio"])
    O.set_mode("exact")
    g = r["keep"]
    assert r["sel"].shape[1] == MI.scored_channels(c) and torch.equal(x[:, ot["order"]], r["sel"])
    rec = dict(c, x_sha256=synth.sha256_tensor(x), ks=r["ks"], K=int(g.numel()), idx_sha256=synth.sha256_tensor(g),
               idx_head=g[:8].tolist(), idx_tail=g[-8:].tolist(), v_sha256=RI.score_sha256(r["v"]),
               f_sha256=RI.score_sha256(r["f"]), chan_sha256=synth.sha256_tensor(ot["order"]), out_sha256=synth.sha256_tensor(x[g]),
               exact_v_sha256=RI.score_sha256(oe["v"]), exact_f_sha256=RI.score_sha256(oe["f"]),
               oracle_torch_mode=dict(ks=ot["ks"] == r["ks"], idx=bool(torch.equal(ot["keep"], g)), chan=True,
                                      scores=bool(torch.equal(ot["v"], r["v"]) and torch.equal(ot["f"], r["f"]))),
               oracle_exact_mode=dict(ks=oe["ks"] == r["ks"], idx=bool(torch.equal(oe["keep"], g)),
                                      scores=bool(torch.equal(oe["v"], r["v"]) and torch.equal(oe["f"], r["f"]))))
    rec.update(premises(c, r["sel"], r["sel"].norm(2, -1), r["v"], r["f"], oe["v"], oe["f"]))
    return rec


def main():
    out = []
    for c in MI.design_cases():
        x = RI.build(c)
        t0 = time.time()
        rec = record(c, x)
        out.append(rec)
        print(c["name"], c["F"], c["N"], c["D"], c["dtype"], f"{time.time() - t0:.1f}s", "norm_ne", rec["norm_ne"], "of",
              c["planted"], "planted, needs_ulps", rec["needs_ulps"], rec["oracle_torch_mode"], flush=True)
    for dn in ("f16", "bf16"):
        need = [r["needs_ulps"] for r in out if r["dtype"] == dn]
        assert sum(32 < n <= 120 for n in need) >= 2 and sum(n > 200 for n in need) >= 2, (dn, need)
    with open(os.path.join(HERE, "margin_cases.json"), "w") as fh:
        json.dump(dict(generator="tests/golden/make_margin_golden.py", torch=torch.__version__, cases=out), fh, indent=None,
                  separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()

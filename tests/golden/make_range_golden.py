#!/usr/bin/env python
"""Range goldens from the REFERENCE (build container only: needs the reference checkout).

    python tests/golden/make_range_golden.py      ->  tests/golden/range_cases.json

Inputs at extreme feature magnitudes (tests/_range_inputs.py: synth.make plus edits written as JSON), where sweep 2
leaves its fast paths for the exact one: norms outside the windows of k_norm_colsum2 / k_norm_colsum, norms below
F.normalize's clamp, fp32 sums of squares that overflow in torch (norm inf, x^ = 0), fp16 norms of inf, fp16-subnormal
rows, bf16 quotients below 2^-125, zero rows, rows inf / NaN in most channels, and LLaVA-Video's grid pass.  Stored as digests (budgets in full; scores with NaN made canonical), plus per case
the premise counts of _range_inputs.counts over the reference's selected channels, and the scale sweeps: for every 2^e of
a range the reference's result is checked against the unscaled clip's, and the exponents where it is unchanged listed.
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
sys.path.insert(0, "/root/reference")

from token_compressor.vidcom2 import vidcom2 as R  # noqa: E402  (the reference)

import _range_inputs as RI  # noqa: E402
import oracle as O  # noqa: E402
from vidcom2_amd import synth  # noqa: E402

torch.set_grad_enabled(False)


def reference(x: torch.Tensor, N: int, base: float):
    sel = R.select_low_var_channels(x)
    v, f = R.compute_gaussian_scores(sel, N)
    scales = R.compute_scales(-v.mean(dim=-1), base)
    ks = (scales * N).round().long().clamp(min=1).tolist()
    g = R._map_linear_offset(R.select_outlier_indices(v + f, scales, N), N)
    return dict(v=v, f=f, ks=ks, g=g, norm=sel.norm(2, -1))


def nan_eq(a, b):
    a, b = a.double(), b.double()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def max_diff(a, b):
    """max |a - b| with NaN against NaN as 0 (NaN against a number stays NaN)."""
    d = (a.double() - b.double()).abs()
    return float(torch.where(a.isnan() & b.isnan(), torch.zeros_like(d), d).max())


def vs_oracle(o, r, x, chan):
    ne = dict(ks=bool(o["ks"].tolist() == r["ks"]), idx=bool(torch.equal(o["global_idx"], r["g"])),
              chan=bool(torch.equal(o["chan_idx"], chan)))
    if x.dtype == torch.float32:
        ne.update(max_dv=max_diff(o["v"], r["v"]), max_df=max_diff(o["f"], r["f"]))
    else:
        ne.update(scores=nan_eq(o["v"], r["v"]) and nan_eq(o["f"], r["f"]))
    return ne


def record(c, x, r):
    g = r["g"]
    chan = RI.low_var_channels(x)
    O.set_mode("exact")
    exact_norm = O.gaussian_debug(x, chan, c["N"])["norm"]
    oe = O.compress_indices(x, c["N"], c["base"])
    O.set_mode("torch")
    ot = O.compress_indices(x, c["N"], c["base"])
    O.set_mode("exact")
    rec = dict(c, x_sha256=synth.sha256_tensor(x), ks=r["ks"], K=int(g.numel()),
               idx_sha256=synth.sha256_tensor(g), idx_head=g[:8].tolist(), idx_tail=g[-8:].tolist(),
               v_sha256=RI.score_sha256(r["v"]), f_sha256=RI.score_sha256(r["f"]),
               chan_sha256=synth.sha256_tensor(chan), out_sha256=synth.sha256_tensor(x[g]),
               counts=RI.counts(x, chan, r["norm"], exact_norm),
               oracle_torch_mode=vs_oracle(ot, r, x, chan), oracle_exact_mode=vs_oracle(oe, r, x, chan))
    if c["dtype"] == "f32":
        rec.update(v_head=r["v"][0, :16].tolist(), f_head=r["f"][0, :16].tolist())
    if c.get("grid_h"):                                   # LLaVA-Video's grid pass end to end (vidcom2.py llava_vid)
        h, img = c["grid_h"], RI.grid_img(c)
        loc = g - torch.repeat_interleave(torch.arange(c["F"]) * c["N"], torch.tensor(r["ks"]))
        gg = R._map_grid_vid(list(torch.split(loc, r["ks"])), h)
        rows = R.vidcom2_compression(x, model="llava_vid", base_scale=c["base"], img_feat=img)
        assert torch.equal(rows, img[gg])
        oracle = {}
        for mode in ("torch", "exact"):
            O.set_mode(mode)
            o = O.vidcom2_compression(x, model="llava_vid", base_scale=c["base"], img_feat=img)
            oracle[mode] = bool(o.shape == rows.shape and torch.equal(o, rows))
        O.set_mode("exact")
        rec.update(img_sha256=synth.sha256_tensor(img), grid_K=int(gg.numel()), grid_idx_sha256=synth.sha256_tensor(gg),
                   grid_out_sha256=synth.sha256_tensor(rows), oracle_grid=oracle)
    return rec


def main():
    out = []
    for c in RI.design_cases():
        x = RI.build(c)
        t0 = time.time()
        r = reference(x, c["N"], c["base"])
        rec = record(c, x, r)
        out.append(rec)
        print(c["name"], c["F"], c["N"], c["D"], c["dtype"], f"{time.time() - t0:.1f}s", "K", rec["K"],
              {k: v for k, v in rec["counts"].items() if v}, rec["oracle_torch_mode"], flush=True)
    sweeps = []
    for s in RI.SWEEPS:
        r0 = reference(RI.sweep_input(s, 0), s["N"], s["base"])
        inv = []
        for e in range(s["e_lo"], s["e_hi"] + 1):
            r = reference(RI.sweep_input(s, e), s["N"], s["base"])
            if nan_eq(r["v"], r0["v"]) and nan_eq(r["f"], r0["f"]) and torch.equal(r["g"], r0["g"]):
                inv.append(e)
        sweeps.append(dict(s, invariant_e=inv, v_sha256=RI.score_sha256(r0["v"]), f_sha256=RI.score_sha256(r0["f"]),
                           idx_sha256=synth.sha256_tensor(r0["g"])))
        print(s["name"], "invariant for", len(inv), "of", s["e_hi"] - s["e_lo"] + 1, "exponents:", inv[0], "..", inv[-1],
              flush=True)
    with open(os.path.join(HERE, "range_cases.json"), "w") as fh:
        json.dump(dict(generator="tests/golden/make_range_golden.py", torch=torch.__version__, cases=out, sweeps=sweeps),
                  fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "cases,", len(sweeps), "sweeps")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Goldens of the pass with non-default hyper-parameters, from the REFERENCE (build container only).

    VIDCOM2_REFERENCE=<checkout of the reference> python tests/golden/make_pass_params_golden.py
                                                            ->  tests/golden/pass_params_cases.json

The reference fixes the share of scored channels (0.5), the softmax temperature (0.01) and the Gaussian scales (2^-3 ..
2^1) in the defaults of its stage functions and in a local list; `vidcom2_compression` passes none of them.  This script
IMPORTS the reference (nothing of its source is copied) and, for the duration of a case, rebinds three globals of its
module: `select_low_var_channels` to a functools.partial with the case's ratio, `compute_scales` to a wrapper with the
case's temp, `_multi_scale_gaussian` to a wrapper that substitutes the case's alphas.  With them rebound it runs the
reference's own `vidcom2_compression` and the stage chain of its hooks (tests/_stage_chain.hook_chain), asserts that the
kept rows of the first are `x[keep]` of the second, and stores the chain's scores, budgets and kept indices as digests
(NaNs canonicalised) and the per-frame vectors in full; inputs are regenerated from the seed at test time.

fp32 cases are admitted by the rule of make_stage_chain_golden.py: the reference's own margins (fp32_margins) above
FP32_TOL, else the next seed; the margins are stored.  Where the CPU oracle has the argument (ratio, temp -- not the
alphas) the record says whether its chain equals the reference's link by link.
"""
from __future__ import annotations

import contextlib
import functools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.environ.get("VIDCOM2_REFERENCE") or sys.argv[1])

from token_compressor.vidcom2 import vidcom2 as R  # noqa: E402  (the reference)

import oracle as O  # noqa: E402
from vidcom2_amd import synth  # noqa: E402

from _stage_chain import DT, FP32_TOL, canon_list, digest, fp32_margins, hook_chain, oracle_chain, same  # noqa: E402

torch.set_grad_enabled(False)

A4 = [0.1, 0.3, 1.0, 3.0]                              # no power of two among them
A8 = [2.0 ** k for k in range(-5, 3)]                  # 2^-5 .. 2^2: the small ones push exp's argument past -16
A16 = [2.0 ** (k / 2) for k in range(-10, 6)]          # 16 scales (the table's capacity), every other one irrational


def C(name, F, N, D, dtype, dist, seed, base=0.25, ratio=None, temp=None, alphas=None, model="linear"):
    return dict(name=name, F=F, N=N, D=D, dtype=dtype, dist=dist, seed=seed, base=base, ratio=ratio, temp=temp,
                alphas=alphas, model=model)


CASES = [
    C("default", 8, 196, 1024, "bf16", "drift", 200),
    # alphas alone (channels and temp at the reference's values: the default sweeps, the table epilogue)
    C("a1", 6, 100, 1024, "f16", "drift", 201, alphas=[1.0]),
    C("a1", 8, 196, 3584, "bf16", "cancel", 202, alphas=[1.0]),
    C("a_ints", 8, 144, 1536, "bf16", "cancel", 203, alphas=[1, 2]),
    C("a_twice", 6, 196, 1024, "f16", "iid", 204, alphas=[0.5, 0.5]),
    C("a4", 8, 196, 3584, "bf16", "drift", 205, alphas=A4),
    C("a4", 6, 100, 1024, "f32", "drift", 206, alphas=A4),
    C("a4", 12, 144, 1536, "f16", "cancel", 207, 0.15, alphas=A4),
    C("a8", 8, 324, 1536, "bf16", "drift", 208, alphas=A8),
    C("a8", 6, 196, 3584, "f16", "cancel", 209, alphas=A8),
    C("a8", 6, 196, 1024, "f32", "iid", 210, alphas=A8),
    C("a16", 6, 100, 1024, "bf16", "iid", 211, alphas=A16),
    C("a16", 16, 144, 1536, "f16", "drift", 212, 0.3, alphas=A16),
    # ratio x temp (the oracle has both arguments)
    C("rt", 12, 196, 1024, "bf16", "drift", 213, ratio=0.25, temp=0.05),
    C("rt", 8, 100, 3584, "f16", "cancel", 214, ratio=0.75, temp=0.5),
    C("rt", 6, 144, 1536, "bf16", "cancel", 215, 0.3, ratio=1.0, temp=1.0),
    C("rt", 6, 196, 1024, "f32", "drift", 216, ratio=0.25, temp=0.5),
    # ratio x temp x alphas
    C("rta", 8, 196, 3584, "bf16", "cancel", 217, ratio=0.25, temp=0.05, alphas=A4),
    C("rta", 6, 144, 1536, "f16", "drift", 218, ratio=0.75, temp=0.5, alphas=[1.0]),
    C("rta", 6, 100, 1024, "bf16", "drift", 219, ratio=1.0, temp=1.0, alphas=A8),
    C("rta", 8, 196, 3584, "f16", "iid", 220, ratio=1 / 128, temp=0.05, alphas=[1, 2]),
    C("rta", 16, 324, 1536, "bf16", "drift", 221, 0.15, ratio=0.75, temp=0.05, alphas=A16),
    C("rta", 6, 196, 1024, "f32", "drift", 222, ratio=0.25, temp=0.05, alphas=[0.5, 0.5]),
    # LLaVA-Video: 13 x 13 tokens per frame scored, rows taken from the 13 x 14 grid (with its newline column)
    C("llava_vid", 8, 169, 1024, "bf16", "drift", 223, ratio=0.25, temp=0.05, alphas=A4, model="llava_vid"),
]


def make_input(c):
    return synth.make(c["F"], c["N"], c["D"], DT[c["dtype"]], c["seed"], c["dist"])


def make_img(c):
    """The grid_vid case's img_feat: [F * 13 * 14, D] from the seed behind the case's own."""
    return synth.make(c["F"], 13 * 14, c["D"], DT[c["dtype"]], c["seed"] + 5000, c["dist"])


@contextlib.contextmanager
def rebound(ratio, temp, alphas):
    """The reference module with a case's hyper-parameters in place of its defaults."""
    saved = (R.select_low_var_channels, R.compute_scales, R._multi_scale_gaussian)
    try:
        if ratio is not None:
            R.select_low_var_channels = functools.partial(saved[0], ratio=ratio)
        if temp is not None:
            R.compute_scales = lambda scores, base: saved[1](scores, base, temp)
        if alphas is not None:
            R._multi_scale_gaussian = lambda x, center, _alphas: saved[2](x, center, alphas)
        yield
    finally:
        R.select_low_var_channels, R.compute_scales, R._multi_scale_gaussian = saved


def links_equal(o, r, fp32):
    eq = dict(sel=same(o["sel"], r["sel"]), ks=o["ks"] == r["ks"], keep=bool(torch.equal(o["keep"], r["keep"])))
    if fp32:
        for k in ("v", "f", "s", "scales"):
            eq["max_d" + k] = float((o[k].double() - r[k].double()).abs().max())
    else:
        eq.update({k: same(o[k], r[k]) for k in ("v", "f", "s", "total", "scales")})
    return eq


def one(c):
    x = make_input(c)
    N, fp32 = c["N"], c["dtype"] == "f32"
    rec = dict(c, x_sha256=synth.sha256_tensor(x))
    with rebound(c["ratio"], c["temp"], c["alphas"]):
        r = hook_chain(R, x, N, c["base"])
        if c["model"] == "llava_vid":
            img = make_img(c)
            gidx = R._map_grid_vid(r["idx"], R.MODEL_SPECS["llava_vid"]["grid"])
            rows = R.vidcom2_compression(x, "llava_vid", c["base"], img_feat=img)
            assert same(rows, img[gidx])
            rec.update(img_sha256=synth.sha256_tensor(img), gidx_sha256=digest(gidx), K_grid=int(gidx.numel()))
        else:
            rows = R.vidcom2_compression(x, "qwen2_5_vl", c["base"], frame_token_len=N)
            assert same(rows, x[r["keep"]])
    assert r["sel"].shape[1] == int(c["D"] * (0.5 if c["ratio"] is None else c["ratio"]))
    if fp32:
        gap, half = fp32_margins(r["total"], r["scales"], r["ks"], N)
        if not (gap > FP32_TOL and half > N * FP32_TOL):
            return None
        rec.update(margin_gap=gap, margin_half=half, v_head=r["v"][0, :16].tolist(), f_head=r["f"][0, :16].tolist())
    rec.update(v_sha256=digest(r["v"]), f_sha256=digest(r["f"]), s=canon_list(r["s"]), scales=canon_list(r["scales"]),
               ks=r["ks"], K=int(r["keep"].numel()), keep_sha256=digest(r["keep"]), rows_sha256=digest(rows), oracle={})
    if c["alphas"] is None:                               # (the oracle's Gaussian has the reference's five scales)
        for mode in ("torch", "exact"):
            O.set_mode(mode)
            rec["oracle"][mode] = links_equal(oracle_chain(x, N, c["base"], c["ratio"], c["temp"]), r, fp32)
        O.set_mode("exact")
    print(c["name"], c["F"], N, c["D"], c["dtype"], c["dist"], c["seed"], "K", rec["K"], rec["oracle"], flush=True)
    return rec


def main():
    out = []
    for c in CASES:
        rec = one(c)
        while rec is None:                                  # (fp32 only: the reference's own margins, see above)
            assert c["seed"] < 20000, "no seed with the margins"
            c = dict(c, seed=c["seed"] + 1000)
            print("  margins too small: next seed", c["seed"], flush=True)
            rec = one(c)
        out.append(rec)
    with open(os.path.join(HERE, "pass_params_cases.json"), "w") as fh:
        json.dump(dict(generator="tests/golden/make_pass_params_golden.py", torch=torch.__version__, fp32_tol=FP32_TOL,
                       cases=out), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()

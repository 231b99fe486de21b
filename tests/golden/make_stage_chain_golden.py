#!/usr/bin/env python
"""Stage-chain goldens from the REFERENCE (build container only: needs /root/reference).

    python tests/golden/make_stage_chain_golden.py      ->  tests/golden/stage_chain_cases.json

The reference's Qwen2.5-VL and Qwen3-VL hooks do not call `vidcom2_compression`: their `_compute_keep_indices` calls the
five stage functions one after the other, with `-v.mean(dim=-1)` and `v + f` of the caller's in between
(tests/_stage_chain.hook_chain).  This script runs that chain FROM THE REFERENCE MODULE and stores every link: channel
order, selected features, both scores, per-frame uniqueness, scales, budgets, kept indices -- as digests (NaNs
canonicalised), the per-frame vectors in full; inputs are regenerated from the seed at test time.  Per case and oracle
mode it records whether the oracle's chain (tests/_stage_chain.oracle_chain) equals the reference link by link.

fp32 cases are compared exactly in budgets and kept indices, so they are admitted only where the reference's own numbers
leave room: the smallest gap between the k-th and (k+1)-th smallest total score of a frame must exceed FP32_TOL and every
scales * tpf must be further than tpf * FP32_TOL from a half-integer; otherwise the next seed is taken.  Both margins are
stored.  For the `var` cases the distance of the reference's x.var(dim=0, unbiased=False) from the fp64 variance is
stored in ulps of the dtype: the bound the stand-alone variance kernel is held to.  Nothing of the reference's source is
copied.
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

import oracle as O  # noqa: E402
from vidcom2_amd import synth  # noqa: E402

from _stage_chain import DT, FP32_TOL, canon_list, case_input, digest, fp32_margins, hook_chain, oracle_chain, same, ulps_of  # noqa: E402

torch.set_grad_enabled(False)


def C(name, F, N, D, dtype, dist, seed, base=0.25, ratio=None, temp=None, var=False):
    return dict(name=name, F=F, N=N, D=D, dtype=dtype, dist=dist, seed=seed, base=base, ratio=ratio, temp=temp, var=var)


CASES = [
    # model widths at hook-like frames: the generic k_norm_colsum<ACC = 1> at C = D / 2 with the identity column order,
    # every frame mean through margin -> flag -> replay
    C("w1536", 8, 144, 1536, "bf16", "drift", 100), C("w1536", 8, 144, 1536, "f16", "cancel", 101),
    C("w1536", 8, 144, 1536, "f16", "iid", 102),
    C("w2048", 6, 260, 2048, "bf16", "cancel", 103), C("w2048", 6, 260, 2048, "f16", "drift", 104, 0.15),
    C("w2560", 6, 391, 2560, "bf16", "drift", 105, 0.3), C("w2560", 6, 391, 2560, "f16", "cancel", 106),
    C("w3584", 8, 324, 3584, "bf16", "drift", 107), C("w3584", 8, 324, 3584, "f16", "cancel", 108, 0.15),
    C("w3584", 8, 324, 3584, "bf16", "cancel", 109),
    C("w4096", 4, 576, 4096, "bf16", "drift", 110), C("w4096", 4, 576, 4096, "f16", "cancel", 111),
    C("w5120", 4, 180, 5120, "bf16", "cancel", 112), C("w5120", 4, 180, 5120, "f16", "drift", 113, 0.3),
    C("w7168", 4, 196, 7168, "bf16", "drift", 114), C("w7168", 4, 196, 7168, "f16", "cancel", 115),
    C("w8192", 3, 100, 8192, "bf16", "drift", 116), C("w8192", 3, 100, 8192, "f16", "cancel", 117),
    C("w8192", 3, 100, 8192, "bf16", "iid", 118),
    C("qwen1296", 4, 1296, 2048, "bf16", "drift", 119), C("qwen1296", 4, 1296, 2048, "f16", "cancel", 120),
    # fp32 (64-bit selection words, fp64 accumulation); D = 4096 is the fp32 row limit
    C("f32", 6, 196, 1024, "f32", "drift", 121), C("f32", 12, 144, 2048, "f32", "iid", 122),
    C("f32_rowlimit", 4, 100, 4096, "f32", "drift", 123),
    # scalar rows: C = 500 / 511, VEC == 1 in every sweep and in the column gather
    C("scalar", 5, 169, 1001, "bf16", "drift", 124), C("scalar", 3, 49, 1022, "f32", "iid", 125),
    # vc2_chan_var's plan of ONE frame of R tokens at clip length (its own stat_splits / rows_per_group / stat_lanes)
    C("clip512", 512, 196, 512, "bf16", "drift", 126, var=True),
    C("target", 128, 196, 3584, "bf16", "drift", 127, var=True), C("target", 128, 196, 3584, "f16", "cancel", 128, var=True),
    # long frames through the stage calls: wave_column_solo, the cascade's second and third level, four-wave selection
    C("n4097", 2, 4097, 328, "f16", "cancel", 129), C("n1021", 4, 1021, 200, "bf16", "drift", 130),
    C("n8192", 3, 8192, 256, "bf16", "drift", 131),
    # degenerate shapes and values
    C("one_token", 1, 1, 64, "bf16", "iid", 132), C("one_token_frames", 3, 1, 64, "f16", "iid", 133),
    C("one_frame", 1, 7, 128, "bf16", "drift", 134), C("one_frame", 1, 7, 128, "f32", "drift", 135),
    C("const", 4, 50, 256, "bf16", "const", 0), C("const", 4, 50, 256, "f16", "const", 0),
    C("zero_rows", 4, 49, 256, "f16", "zrows", 136),          # NaN scores, NaN scales, budgets of 1
    # budgets: a few tokens per frame; scales clamped at 1 (a frame kept whole)
    C("base0.05", 16, 196, 3584, "bf16", "drift", 137, 0.05), C("base0.6", 16, 196, 3584, "f16", "drift", 138, 0.6),
    # ratio: k * 64 <= D -> libstdc++ partial_sort; 0.25 / 0.75 -> nth_element + sort; 1.0 -> k = D, everything sorted
    C("ratio", 6, 100, 3584, "bf16", "drift", 139, ratio=1 / 128), C("ratio", 6, 100, 3584, "f16", "drift", 140, ratio=0.25),
    C("ratio", 6, 100, 3584, "bf16", "cancel", 141, ratio=0.75), C("ratio", 6, 100, 3584, "f16", "cancel", 142, ratio=1.0),
    C("ratio", 6, 196, 1024, "f16", "drift", 143, ratio=1 / 128), C("ratio", 6, 196, 1024, "bf16", "drift", 144, ratio=0.25),
    C("ratio", 6, 196, 1024, "f32", "drift", 145, ratio=0.75), C("ratio", 6, 196, 1024, "bf16", "iid", 146, ratio=1.0),
    # temp: the softmax of compute_scales away from 0.01
    C("temp", 8, 196, 1024, "bf16", "drift", 147, temp=0.05), C("temp", 8, 196, 1024, "f16", "drift", 148, temp=0.5),
    C("temp", 8, 196, 1024, "f32", "drift", 149, temp=1.0), C("temp", 16, 144, 3584, "bf16", "drift", 150, 0.3, temp=0.05),
]

# vc2_chan_var alone at row counts that are a multiple of nothing
VAR_CASES = [C("var_r25087", 1, 25087, 3584, "bf16", "drift", 160, var=True),
             C("var_r25087", 1, 25087, 3584, "f16", "iid", 161, var=True),
             C("var_r33", 3, 11, 1001, "bf16", "drift", 162, var=True), C("var_r33", 3, 11, 1001, "f32", "iid", 163, var=True)]


def make_input(F, N, D, dn, seed, dist):
    return synth.make(F, N, D, DT[dn], seed, dist)


def variance(c, x, rec):
    var = x.var(dim=0, unbiased=False)
    rec["var_sha256"] = digest(var)
    if c["var"]:
        rec["var_ulps_vs_fp64"] = ulps_of(x.dtype, var, x.double().var(dim=0, unbiased=False))
    return var


def links_equal(o, r, order, fp32):
    """The oracle's chain against the reference's, link by link: True / False, for fp32 scores the largest difference."""
    eq = dict(order=bool(torch.equal(o["order"], order)), sel=same(o["sel"], r["sel"]), ks=o["ks"] == r["ks"],
              keep=bool(torch.equal(o["keep"], r["keep"])))
    if fp32:
        for k in ("v", "f", "s", "scales"):
            eq["max_d" + k] = float((o[k].double() - r[k].double()).abs().max())
    else:
        eq.update({k: same(o[k], r[k]) for k in ("v", "f", "s", "total", "scales")})
    return eq


def one(c):
    x = case_input(c, make_input)
    N, fp32 = c["N"], c["dtype"] == "f32"
    t0 = time.time()
    r = hook_chain(R, x, N, c["base"], c["ratio"], c["temp"])
    dt_ref = time.time() - t0
    rec = dict(c, x_sha256=synth.sha256_tensor(x))
    var = variance(c, x, rec)
    order = torch.topk(var, k=int(c["D"] * (0.5 if c["ratio"] is None else c["ratio"])), largest=False)[1]
    assert torch.equal(x[:, order], r["sel"])
    ks_ref = (r["scales"] * N).round().long().clamp(min=1).tolist()
    assert ks_ref == r["ks"]
    if fp32:
        gap, half = fp32_margins(r["total"], r["scales"], r["ks"], N)
        if not (gap > FP32_TOL and half > N * FP32_TOL):
            return None
        rec.update(margin_gap=gap, margin_half=half, v_head=r["v"][0, :16].tolist(), f_head=r["f"][0, :16].tolist())
    rec.update(order_sha256=digest(order), sel_sha256=digest(r["sel"]), v_sha256=digest(r["v"]), f_sha256=digest(r["f"]),
               s=canon_list(r["s"]), scales=canon_list(r["scales"]), ks=r["ks"], K=int(r["keep"].numel()),
               keep_sha256=digest(r["keep"]), oracle={})
    for mode in ("torch", "exact"):
        O.set_mode(mode)
        t0 = time.time()
        rec["oracle"][mode] = links_equal(oracle_chain(x, N, c["base"], c["ratio"], c["temp"]), r, order, fp32)
        dt_o = time.time() - t0
    O.set_mode("exact")
    print(c["name"], c["F"], N, c["D"], c["dtype"], c["dist"], c["seed"], "K", rec["K"], f"reference {dt_ref:.1f}s oracle {dt_o:.1f}s",
          rec["oracle"], flush=True)
    return rec


def main():
    out, var_out = [], []
    for c in CASES:
        rec = one(c)
        while rec is None:                                  # (fp32 only: the reference's own margins, see above)
            assert c["seed"] < 20000, "no seed with the margins"
            c = dict(c, seed=c["seed"] + 1000)
            print("  margins too small: next seed", c["seed"], flush=True)
            rec = one(c)
        out.append(rec)
    for c in VAR_CASES:
        x = case_input(c, make_input)
        rec = dict(c, x_sha256=synth.sha256_tensor(x))
        variance(c, x, rec)
        var_out.append(rec)
        print(c["name"], c["dtype"], "var ulps vs fp64", rec["var_ulps_vs_fp64"], flush=True)
    with open(os.path.join(HERE, "stage_chain_cases.json"), "w") as fh:
        json.dump(dict(generator="tests/golden/make_stage_chain_golden.py", torch=torch.__version__, fp32_tol=FP32_TOL,
                       cases=out, var_cases=var_out), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "chain cases,", len(var_out), "variance cases")


if __name__ == "__main__":
    main()

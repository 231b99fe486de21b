#!/usr/bin/env python
"""Goldens of the fp32-scored pass over 16-bit inputs, from the REFERENCE (build container only).

    VIDCOM2_REFERENCE=<checkout of the reference> python tests/golden/make_score_dtype_golden.py
                                                            ->  tests/golden/score_dtype_cases.json

`compress(x, ..., score_dtype=torch.float32)` on a bf16 / fp16 tensor is the reference applied to x.float().  This script
IMPORTS the reference (nothing of its source is copied), runs its own stage chain and `vidcom2_compression` on the widened
`synth` input of every candidate (tests/_score_dtype.candidates) and records: shape, storage dtype, dist, seed, base,
mapper, x_sha256, ks, global_idx, the first 16 v / f values of frame 0, the smallest decision margin, and native_overlap --
the fraction of the fp32-scored kept set that the reference run in the STORAGE dtype also keeps (SURVEY.md finding 2).
The two cases with non-default hyper-parameters rebind the reference's globals as make_pass_params_golden.py does.

Admission (a condition, not a measurement): a candidate is written only if
  * the reference, the CPU oracle in `exact` mode and in `torch` mode agree on ks and global_idx for the widened input, and
  * its smallest decision margin -- the gap between the k-th and (k+1)-th smallest v + f of any frame with 0 < k < N -- is
    at least MARGIN_MIN = 5e-6: five times the 1e-6 score tolerance, so two scores each off by it cannot swap.
Fewer than 90 % of the candidates admitted is an error.
"""
from __future__ import annotations

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

import _score_dtype as SD  # noqa: E402
from _stage_chain import hook_chain, same  # noqa: E402
from make_pass_params_golden import rebound  # noqa: E402

torch.set_grad_enabled(False)


def one(c):
    x = SD.make_input(c)
    x32 = x.float()
    N = c["N"]
    with rebound(c["ratio"], c["temp"], c["alphas"]):
        r = hook_chain(R, x32, N, c["base"])              # the reference on the widened input
        native = hook_chain(R, x, N, c["base"])           # ... and in the storage dtype
        if c["mapper"] == "grid_vid":
            img = SD.make_img(c)
            gidx = R._map_grid_vid(r["idx"], SD.grid_h(c))
            assert same(R.vidcom2_compression(x32, "llava_vid", c["base"], img_feat=img.float()), img.float()[gidx])
        else:
            gidx = r["keep"]
            assert same(R.vidcom2_compression(x32, "qwen2_5_vl", c["base"], frame_token_len=N), x32[gidx])
    agree = True
    for mode in ("exact", "torch"):
        O.set_mode(mode)
        o = SD.oracle_pass(x32, c)
        agree = agree and o["ks"] == r["ks"] and bool(torch.equal(o["keep"], r["keep"]))
    O.set_mode("exact")
    margin = SD.decision_margin(r["total"], r["ks"])
    ok = agree and (margin is None or margin >= SD.MARGIN_MIN)
    kept = set(r["keep"].tolist())
    overlap = len(kept & set(native["keep"].tolist())) / max(1, len(kept))
    print(SD.case_id(c), "K", len(kept), "margin", margin, "oracle agrees", agree, "native overlap", round(overlap, 3),
          "" if ok else "-> DROPPED", flush=True)
    if not ok:
        return None
    return dict(c, x_sha256=synth.sha256_tensor(x), ks=r["ks"], global_idx=gidx.tolist(), K=int(gidx.numel()),
                v_head=r["v"][0, :16].tolist(), f_head=r["f"][0, :16].tolist(), margin=margin, native_overlap=overlap)


def main():
    cands = SD.candidates()
    out = [rec for rec in map(one, cands) if rec is not None]
    assert len(out) >= 0.9 * len(cands), f"only {len(out)} of {len(cands)} candidates admitted"
    with open(SD.GOLDEN, "w") as fh:
        json.dump(dict(generator="tests/golden/make_score_dtype_golden.py", torch=torch.__version__,
                       margin_min=SD.MARGIN_MIN, candidates=len(cands), cases=out), fh, indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "of", len(cands), "candidates")


if __name__ == "__main__":
    main()

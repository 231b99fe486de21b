#!/usr/bin/env python
"""Long-frame goldens from the REFERENCE (build container only: needs /root/reference).

    python tests/golden/make_long_frame_golden.py      ->  tests/golden/long_frame_cases.json

Frames of 256 to 8192 tokens (the library's limit), where the kernels switch code paths on N: the frame-mean replay
(lds_column_short up to 512 rows, wave_column_solo above), torch's cascade levels (a second level at 256 rows, at 1024 in
the tail columns' four chains, a third at 4096), sweep 2's ORD form (N <= 512), the selection engines (solo<4> / <8>,
one-wave up to 1020 values, four-wave up to 8188 cooperatively) and the plan geometry.  Qwen2/2.5/3-VL frames at
ordinary resolutions have 576 to 1296 tokens.

Stored as digests (budgets in full); inputs are regenerated from the seed at test time (vidcom2_amd/synth.py).  Per
case the script records how many frame-centre and video-centre means of the oracle's `exact` mode (fp64 sums) differ
from the reference's own, and how many of those frame means lie in tail columns (C % 32 != 0).  A case with non-zero
counts is one where torch's summation order decides a centre: a HIP pass that skipped or misordered a replay fails it.  Nothing of the reference's source is copied.
"""
from __future__ import annotations

import json
import os
import sys
import time

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

from token_compressor.vidcom2 import vidcom2 as R  # noqa: E402  (the reference)

import oracle as O  # noqa: E402
from vidcom2_amd import synth  # noqa: E402

torch.set_grad_enabled(False)
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

CASES = [  # name, F, N, D, dtype, dist, seed, base
    ("n256", 4, 256, 1024, "bf16", "drift", 0, 0.25),        # topk_smallest4_solo<4>; ORD <16>; one cascade level
    ("n257", 4, 257, 1024, "bf16", "drift", 1, 0.25),        # solo<8>; ORD <33>; a second level (and one row after it)
    ("n256", 4, 256, 1024, "f16", "drift", 2, 0.25),
    ("n257", 4, 257, 1024, "f16", "drift", 3, 0.25),
    ("n512", 3, 512, 3584, "bf16", "drift", 4, 0.25),        # the last ORD shape, lds_column_short, solo<8>
    ("n512", 3, 512, 3584, "f16", "drift", 5, 0.25),
    ("n512", 3, 512, 3584, "f16", "cancel", 6, 0.25),
    ("n513", 3, 513, 3584, "bf16", "drift", 7, 0.25),        # margin / flag / replay form, wave_column_solo, one-wave select
    ("n513", 3, 513, 3584, "f16", "drift", 8, 0.25),
    ("n513", 3, 513, 3584, "f16", "cancel", 9, 0.25),
    ("qwen576", 3, 576, 3584, "bf16", "drift", 10, 0.25),    # Qwen2.5-VL frames at model width
    ("qwen576", 3, 576, 3584, "f16", "cancel", 11, 0.25),
    ("qwen1296", 3, 1296, 3584, "bf16", "drift", 12, 0.25),
    ("qwen1296", 3, 1296, 3584, "f16", "cancel", 13, 0.25),
    ("n1020", 6, 1020, 1024, "bf16", "drift", 14, 0.25),     # sel2_capacity(1, 4): the last one-wave selection
    ("n1020", 6, 1020, 200, "f16", "cancel", 15, 0.25),      # C = 100: columns 96.. are tail columns
    ("n1021", 6, 1021, 200, "f32", "iid", 16, 0.25),         # the first four-wave selection
    ("n1021", 6, 1021, 1024, "f16", "cancel", 17, 0.25),
    ("n1021", 6, 1021, 200, "bf16", "drift", 18, 0.25),
    ("n1024", 6, 1024, 200, "f16", "cancel", 19, 0.25),      # row_sum's four chains of 256: their second level
    ("n1024", 6, 1024, 1024, "f32", "iid", 20, 0.25),
    ("n1024", 6, 1024, 1024, "bf16", "drift", 21, 0.25),
    ("n4095", 2, 4095, 4096, "bf16", "drift", 22, 0.25),     # one row short of the third cascade level
    ("n4096", 6, 4096, 328, "f16", "cancel", 23, 0.25),      # the third level; C = 164: tail columns
    ("n4096", 2, 4096, 4096, "f16", "cancel", 24, 0.25),
    ("n4097", 6, 4097, 328, "bf16", "drift", 25, 0.25),
    ("n4097", 2, 4097, 4096, "f16", "cancel", 26, 0.25),
    ("n8188", 4, 8188, 256, "bf16", "drift", 27, 0.25),      # sel2_capacity(4, 8): the four-wave cooperative capacity
    ("n8189", 4, 8189, 256, "f16", "cancel", 28, 0.25),      # one past it
    ("n8189", 3, 8189, 256, "f32", "iid", 29, 0.25),
    ("n8192", 4, 8192, 256, "bf16", "drift", 30, 0.25),      # the library's limit
    ("n8192", 4, 8192, 256, "f16", "cancel", 31, 0.25),
    ("n8192", 2, 8192, 256, "f32", "iid", 32, 0.25),         # fp32: 64-bit selection words
    ("n8192", 1, 8192, 3584, "bf16", "drift", 33, 0.25),
    ("n8192", 1, 8192, 3584, "f16", "cancel", 34, 0.25),
    ("n8192", 2, 8192, 328, "f16", "cancel", 35, 0.25),
    ("sharded1296", 6, 1296, 3584, "f16", "cancel", 39, 0.25),   # the frame-sharded pass (2 and 3 ranks)
    ("k1", 5, 4097, 1024, "bf16", "drift", 36, 0.0001),      # every budget 1
    ("base0.005", 5, 1021, 1024, "f16", "drift", 37, 0.005),
    ("base1", 5, 1021, 1024, "bf16", "drift", 38, 1.0),      # budgets of N in the frames the softmax favours
]


def reference(x: torch.Tensor, N: int, base: float):
    """The reference's stages, called one by one so that its centres can be read off too."""
    sel = R.select_low_var_channels(x)
    v, f = R.compute_gaussian_scores(sel, N)
    scales = R.compute_scales(-v.mean(dim=-1), base)
    ks = (scales * N).round().long().clamp(min=1).tolist()
    g = R._map_linear_offset(R.select_outlier_indices(v + f, scales, N), N)
    frames = F.normalize(sel.view(-1, N, sel.shape[-1]), dim=-1)
    return dict(v=v, f=f, ks=ks, g=g, frame_centre=frames.mean(dim=1), video_centre=frames.mean(dim=(0, 1)))


def vs_oracle(o, r, x, chan):
    ne = dict(ks=bool(o["ks"].tolist() == r["ks"]), idx=bool(torch.equal(o["global_idx"], r["g"])),
              chan=bool(torch.equal(o["chan_idx"], chan)))
    if x.dtype == torch.float32:
        ne.update(max_dv=float((o["v"].double() - r["v"].double()).abs().max()),
                  max_df=float((o["f"].double() - r["f"].double()).abs().max()))
    else:
        ne.update(v_mismatch=int((o["v"].double() != r["v"].double()).sum()),
                  f_mismatch=int((o["f"].double() != r["f"].double()).sum()))
    return ne


def main():
    out = []
    for name, Fr, N, D, dn, dist, seed, base in CASES:
        x = synth.make(Fr, N, D, DT[dn], seed, dist)
        t0 = time.time()
        r = reference(x, N, base)
        dt_ref = time.time() - t0
        g = r["g"]
        chan = torch.topk(x.var(dim=0, unbiased=False), k=int(D * 0.5), largest=False)[1]
        O.set_mode("exact")
        dbg = O.gaussian_debug(x, chan, N)
        ne_f, ne_v = dbg["frame_center"] != r["frame_centre"], dbg["vid_center"] != r["video_centre"]
        tail = (chan.numel() // 32) * 32                     # columns from here on take row_sum's four chains
        oe = O.compress_indices(x, N, base)
        O.set_mode("torch")
        ot = O.compress_indices(x, N, base)
        O.set_mode("exact")
        rec = dict(name=name, F=Fr, N=N, D=D, base=base, dtype=dn, dist=dist, seed=seed,
                   x_sha256=synth.sha256_tensor(x), ks=r["ks"], K=int(g.numel()),
                   idx_sha256=synth.sha256_tensor(g), idx_head=g[:8].tolist(), idx_tail=g[-8:].tolist(),
                   v_sha256=synth.sha256_tensor(r["v"]), f_sha256=synth.sha256_tensor(r["f"]),
                   chan_sha256=synth.sha256_tensor(chan), out_sha256=synth.sha256_tensor(x[g]),
                   centres_exact_ne=dict(frame=int(ne_f.sum()), video=int(ne_v.sum()),
                                         frame_tail_columns=int(ne_f[:, tail:].sum())),
                   oracle_torch_mode=vs_oracle(ot, r, x, chan), oracle_exact_mode=vs_oracle(oe, r, x, chan))
        if dn == "f32":
            rec.update(v_head=r["v"][0, :16].tolist(), f_head=r["f"][0, :16].tolist())
        out.append(rec)
        print(name, Fr, N, D, dn, dist, seed, base, "K", rec["K"], f"reference {dt_ref:.1f}s",
              rec["centres_exact_ne"], rec["oracle_torch_mode"], flush=True)
        del x, r, dbg, oe, ot
    with open(os.path.join(HERE, "long_frame_cases.json"), "w") as fh:
        json.dump(dict(generator="tests/golden/make_long_frame_golden.py", torch=torch.__version__, cases=out), fh,
                  indent=None, separators=(",", ":"))
        fh.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()

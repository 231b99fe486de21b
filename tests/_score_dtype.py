"""Shared by tests/golden/make_score_dtype_golden.py and the score_dtype tests: the fixture's candidate cases, their
inputs, and the CPU oracle's pass over the WIDENED input (x.float()) -- TEST ONLY.

The fp32-scored pass (`compress(x, ..., score_dtype=torch.float32)` on a bf16 / fp16 tensor) is the reference applied to
x.float(); tests/golden/score_dtype_cases.json records what the reference itself keeps there."""
import json
import os

import torch

import oracle as O
from vidcom2_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "score_dtype_cases.json")
DT = {"bf16": torch.bfloat16, "f16": torch.float16}

SCORE_TOL = 1e-6          # the pass's scores against the oracle's (DESIGN.md "Numerics contract", fp32)
HEAD_TOL = 1e-5           # ... and against the reference's recorded heads
MARGIN_MIN = 5e-6         # admission: five times SCORE_TOL, so two scores each off by the tolerance cannot swap

# the smallest shapes at which each kernel path can go wrong
SHAPES = [
    (4, 49, 64),          # a row narrower than one wave of vectors
    (3, 50, 100),         # 200-byte rows: the scalar path
    (5, 33, 256),         # odd N
    (16, 169, 512),       # two 8-frame stat blocks
    (2, 257, 1024),       # N > 256: more than one token per selection thread
    (1, 64, 128),         # F = 1
    (8, 196, 1024),       # the smoke shape
    (2, 196, 3584),       # model width, 1792 scored channels
]
A4 = [0.1, 0.3, 1.0, 3.0]


def _case(F, N, D, dtype, dist, seed, base=0.25, mapper="linear", ratio=None, temp=None, alphas=None):
    return dict(F=F, N=N, D=D, dtype=dtype, dist=dist, seed=seed, base=base, mapper=mapper, ratio=ratio, temp=temp,
                alphas=alphas)


def candidates():
    out = [_case(F, N, D, dt, dist, seed) for (F, N, D) in SHAPES for dt in ("bf16", "f16") for dist in ("drift", "iid")
           for seed in (0, 1)]
    out.append(_case(16, 169, 512, "bf16", "drift", 0, mapper="grid_vid"))      # h = 13, img_feat of F * 13 * 14 rows
    out.append(_case(1, 64, 128, "bf16", "drift", 0, base=0.01))                # k = 1: the k * 64 <= N heap-select regime
    out.append(_case(1, 64, 128, "bf16", "drift", 0, base=1.0))                 # k = N
    out.append(_case(4, 49, 64, "bf16", "drift", 0, ratio=0.25, temp=0.05, alphas=A4))
    out.append(_case(5, 33, 256, "f16", "drift", 0, ratio=0.75, alphas=[1.0]))
    return out


def case_id(c):
    tag = f"{c['F']}x{c['N']}x{c['D']}-{c['dtype']}-{c['dist']}{c['seed']}-b{c['base']}"
    if c["mapper"] != "linear":
        tag += "-" + c["mapper"]
    if has_params(c):
        tag += f"-r{c['ratio']}-t{c['temp']}-a{len(c['alphas'])}"
    return tag


def has_params(c):
    return c["ratio"] is not None or c["temp"] is not None or c["alphas"] is not None


def make_input(c):
    return synth.make(c["F"], c["N"], c["D"], DT[c["dtype"]], c["seed"], c["dist"])


def make_img(c):
    """A grid_vid case's img_feat: [F * h * (h + 1), D] from the seed behind the case's own."""
    h = grid_h(c)
    return synth.make(c["F"], h * (h + 1), c["D"], DT[c["dtype"]], c["seed"] + 5000, c["dist"])


def grid_h(c):
    h = int(round(c["N"] ** 0.5))
    assert h * h == c["N"]
    return h


def load():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


def oracle_pass(x32, c):
    """The CPU oracle's pass (in the mode it is in) over the widened input: dict(ks, keep -- the LINEAR global indices --,
    v, f, total).  Without params it is the oracle's whole-pass call; with them the stage chain, the Gaussian through the
    oracle's standalone multi-scale call (the only one that takes the scales)."""
    N, base = c["N"], c["base"]
    if not has_params(c):
        o = O.compress_indices(x32, N, base)
        return dict(ks=o["ks"].tolist(), keep=o["global_idx"], v=o["v"], f=o["f"], total=o["total"])
    ratio = 0.5 if c["ratio"] is None else c["ratio"]
    temp = 0.01 if c["temp"] is None else c["temp"]
    order, _ = O.select_low_var_channel_idx(x32, ratio)
    sel = x32[:, order].contiguous()
    if c["alphas"] is None:
        v, f = O.compute_gaussian_scores(sel, N)
    else:
        F, C = c["F"], sel.shape[1]
        dbg = O.gaussian_debug(sel, torch.arange(C), N)
        xn = (sel / dbg["norm"].clamp_min(1e-12)[:, None]).view(F, N, C)        # F.normalize: one IEEE division per element
        v = O.multi_scale_gaussian(xn, dbg["vid_center"].view(1, 1, C), c["alphas"])
        f = O.multi_scale_gaussian(xn, dbg["frame_center"].view(F, 1, C), c["alphas"])
    s, total = O.fuse(v, f)
    scales = O.compute_scales(s, base, temp)
    idx = O.select_outlier_indices(total, scales, N)
    return dict(ks=[int(i.numel()) for i in idx], keep=O.map_linear_offset(idx, N), v=v, f=f, total=total)


def grid_indices(keep, ks, c):
    """The grid_vid global indices (kept tokens in the h x (h + 1) grid, then the frame's h newline rows) from the
    linear ones."""
    N, h = c["N"], grid_h(c)
    loc = keep - torch.repeat_interleave(torch.arange(c["F"]) * N, torch.tensor(ks))
    return O.map_grid_vid(list(torch.split(loc, ks)), h)


def decision_margin(total, ks):
    """The smallest gap between the k-th and (k+1)-th smallest total score of any frame with 0 < k < N (None: no frame
    decides anything)."""
    gap = None
    for row, k in zip(total.double(), ks):
        if 0 < k < row.numel():
            srt = row.sort().values
            g = float(srt[k] - srt[k - 1])
            gap = g if gap is None else min(gap, g)
    return gap

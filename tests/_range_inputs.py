"""Inputs at extreme feature magnitudes, shared by tests/golden/make_range_golden.py and the tests (not a conftest).

Every other fixture comes from vidcom2_amd/synth.py as it is: elements between about 1e-5 and 30, selected-channel norms
between about 10 and 100 -- every row inside the windows of sweep 2's fast paths (k_norm_colsum2: a bf16 norm in
[2^-39, 2^40], an fp16 norm in [2^-14, 32768], bf16 quotients >= 2^-125; k_norm_colsum: bf16 elements in [2^-63, 2^50]).
A case here is synth.make(...) plus a short list of edits that can be written as JSON:

    {"op": "scale", "e": E, "rows": [..] | null}                          x[rows] *= 2^E   (null: every row)
    {"op": "set", "rows": [..] | null, "cols": [..] | null, "value": v}   x[rows, cols] = v   (a T value, "inf", "nan")
    {"op": "add", "cols": [..], "value": c}                               x[:, cols] += c
    {"op": "pattern", "rows": [..] | null, "cols": [..] | null, "head": [..], "tail": [..]}
                                   x[rows, cols[j]] = head[j] for j < len(head), else tail[j % len(tail)]

Each edit is done in fp64 and rounded to T once (a power-of-two scaling is exact unless it leaves T's normal range).
The exponents are chosen from the data (design_cases): where a clip's selected-channel norms sit decides E.  `premise`
names the counts (counts()) that must be non-zero for the case to test what it is meant to."""
from __future__ import annotations

import math

import torch

from vidcom2_amd import synth

DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# the windows of sweep 2's fast paths (vc2_kernels.hip: kS2Norm*, kBf16Span*) and the overflow of torch's fp32 sum of
# squares (FLT_MAX = (2 - 2^-23) 2^127: a norm of 2^64 or more)
BF16_LO, BF16_HI = 2.0 ** -39, 2.0 ** 40
F16_LO, F16_HI = 2.0 ** -14, 32768.0
F16_MAX = 65504.0
FLT_MAX = float(torch.finfo(torch.float32).max)


def apply(x: torch.Tensor, ops) -> torch.Tensor:
    """The edits of `ops` on a copy of x ([R, D], any of the three dtypes)."""
    y = x.clone()
    for o in ops:
        rows = torch.arange(y.shape[0]) if o.get("rows") is None else torch.tensor(o["rows"], dtype=torch.int64)
        cols = torch.arange(y.shape[1]) if o.get("cols") is None else torch.tensor(o["cols"], dtype=torch.int64)
        blk = y[rows[:, None], cols[None, :]].double()
        if o["op"] == "scale":
            blk = blk * (2.0 ** int(o["e"]))
        elif o["op"] == "set":
            blk = torch.full_like(blk, float(o["value"]))
        elif o["op"] == "add":
            blk = blk + float(o["value"])
        elif o["op"] == "pattern":
            head, tail = [float(v) for v in o["head"]], [float(v) for v in o["tail"]]
            line = [head[j] if j < len(head) else tail[j % len(tail)] for j in range(blk.shape[1])]
            blk = torch.tensor(line, dtype=torch.float64).expand_as(blk)
        else:
            raise ValueError(o["op"])
        y[rows[:, None], cols[None, :]] = blk.to(y.dtype)
    return y


def build(c) -> torch.Tensor:
    """The [F * N, D] input of a case (a dict with F, N, D, dtype, seed, dist, ops)."""
    return apply(synth.make(c["F"], c["N"], c["D"], DT[c["dtype"]], c["seed"], c["dist"]), c["ops"])


def score_sha256(t: torch.Tensor) -> str:
    """sha256 of a score tensor with every NaN as the one canonical NaN (which NaN an op returns is not specified)."""
    t = t.detach().cpu().clone()
    t[t.isnan()] = math.nan
    return synth.sha256_tensor(t)


def low_var_channels(x: torch.Tensor) -> torch.Tensor:
    """The reference's selected channels (vidcom2.py select_low_var_channels), in torch.topk's order."""
    return torch.topk(x.var(dim=0, unbiased=False), k=int(x.shape[1] * 0.5), largest=False)[1]


def sel_norms(x: torch.Tensor) -> torch.Tensor:
    """fp64 norms of the rows over the selected channels."""
    return x[:, low_var_channels(x)].double().norm(dim=-1)


def counts(x: torch.Tensor, chan: torch.Tensor, ref_norm: torch.Tensor, exact_norm: torch.Tensor) -> dict:
    """The premise of a case, worked out on the host from the T values over the reference's selected channels: rows
    outside each window, rows whose fp32 sum of squares overflows, rows whose `exact` norm differs from the
    reference's (NaN equal to NaN)."""
    s = x[:, chan].double()
    n = s.norm(dim=-1)
    fin = torch.isfinite(s).all(dim=-1)
    a = s.abs()
    amin = torch.where(a > 0, a, torch.full_like(a, math.inf)).min(dim=-1).values
    amax = a.max(dim=-1).values
    rn, en = ref_norm.double(), exact_norm.double()
    ne = ~((rn == en) | (rn.isnan() & en.isnan()))
    cnt = lambda m: int((fin & m).sum())                            # noqa: E731
    return dict(
        rows=int(x.shape[0]), nonfinite=int((~fin).sum()), zero=cnt(n == 0),
        bf16_norm_below=cnt(n < BF16_LO), bf16_norm_above=cnt(n > BF16_HI),
        bf16_elem_outside=cnt((amin < 2.0 ** -63) | (amax > 2.0 ** 50)),
        bf16_quot_below=cnt((n > 0) & (amin / n < 2.0 ** -125)),
        f16_norm_below=cnt(n < F16_LO), f16_norm_above=cnt(n > F16_HI), f16_norm_over_max=cnt(n > F16_MAX),
        f16_subnormal_rows=cnt(amax < 2.0 ** -14),
        below_clamp=cnt(n < 1e-12),
        fp32_sumsq_overflow=cnt(n * n > FLT_MAX),
        exact_norm_ne=int(ne.sum()),
    )


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _e_above(v, lim):      # the smallest e with v 2^e > lim
    return math.floor(math.log2(lim / v)) + 1


def _e_below(v, lim):      # the largest e with v 2^e < lim
    return math.ceil(math.log2(lim / v)) - 1


def _case(name, fam, F, N, D, dn, seed, ops, premise, dist="drift", base=0.25):
    return dict(name=name, family=fam, F=F, N=N, D=D, dtype=dn, seed=seed, dist=dist, base=base, ops=ops, premise=premise)


def mixed_rows(F, N):
    """Rows of family B: inside one wave and one 16-row ORD block at its first and at its last row, the N % 16
    leftover chain, the first and the last row of a frame -- in frames 0 and F - 1 (the frames between stay ordinary)."""
    rows = []
    for f in (0, F - 1):
        b = f * N
        rows += [b, b + 3, b + 5, b + 16, b + 31, b + N - 1]
        if N % 16:
            rows.append(b + (N // 16) * 16 + 1)
    return sorted(set(rows))


def _scale(e, rows=None):
    return [dict(op="scale", e=int(e), rows=rows)]


# premise of the overflow cases (`exact_norm_ne`: the `exact` norm and the reference's disagree -- a pass that ignored
# torch's overflow would still pass a case without it)
_OVF = ["fp32_sumsq_overflow", "exact_norm_ne"]


def design_cases():
    """The range cases: A whole-clip scaling, B rows scaled among ordinary rows, C offset channels, D bf16 quotients
    below 2^-125, E zero rows and non-finite elements (exponents from the data of each base clip)."""
    out = []
    # ---- A. whole-clip scaling by 2^e --------------------------------------------------------------------------------
    for F, N, D, seed, full in [(8, 196, 3584, 1, True), (4, 196, 1024, 2, False), (3, 576, 3584, 3, False),
                                (3, 196, 1536, 4, False), (2, 197, 1001, 5, False)]:
        n = sel_norms(synth.make(F, N, D, torch.bfloat16, seed, "drift"))
        lo, hi = float(n.min()), float(n.max())
        es = {"hi_in": (_e_below(hi, BF16_HI), []), "hi_out": (_e_above(lo, BF16_HI), ["bf16_norm_above"]),
              "lo_in": (_e_above(lo, BF16_LO), []), "lo_out": (_e_below(hi, BF16_LO), ["bf16_norm_below"]),
              "clamp": (_e_below(hi, 1e-12), ["below_clamp"]), "ovf": (_e_above(lo, 2.0 ** 64), _OVF),
              "ovf_far": (_e_above(lo, 2.0 ** 64) + 6, _OVF)}
        for k, (e, pm) in es.items():
            if full or k in ("hi_out", "ovf"):
                out.append(_case(f"A{D}-bf16-{k}", "A", F, N, D, "bf16", seed, _scale(e), pm))
    for F, N, D, seed, full in [(8, 196, 3584, 6, True), (4, 196, 1024, 7, False), (4, 196, 4096, 8, False),
                                (3, 576, 3584, 9, False), (3, 196, 2048, 10, False),
                                (2, 197, 1001, 29, False)]:
        xs = synth.make(F, N, D, torch.float16, seed, "drift")
        n = sel_norms(xs)
        lo, hi = float(n.min()), float(n.max())
        # (a norm below 2^-14 for every row is out of reach: fp16 variances of such values vanish, and the channels that
        #  are selected then carry larger norms -- family B has such rows among ordinary ones)
        es = {"hi_out": (_e_above(lo, F16_HI), ["f16_norm_above"]), "inf": (_e_above(lo, 65520.0), ["f16_norm_over_max"]),
              "subnormal": (_e_below(float(xs.double().abs().max()), 2.0 ** -14), ["f16_subnormal_rows"])}
        for k, (e, pm) in es.items():
            if full or k in ("hi_out", "inf"):
                out.append(_case(f"A{D}-f16-{k}", "A", F, N, D, "f16", seed, _scale(e), pm))
    n = sel_norms(synth.make(4, 196, 1024, torch.float32, 11, "iid"))
    e = _e_above(float(n.min()), 2.0 ** 64)
    out += [_case("A1024-f32-ovf", "A", 4, 196, 1024, "f32", 11, _scale(e), _OVF, "iid"),
            _case("A1024-f32-ovf_far", "A", 4, 196, 1024, "f32", 11, _scale(e + 6), _OVF, "iid")]
    # ---- B. some rows out of the window among ordinary rows -----------------------------------------------------------
    for F, N, D, dn, seed in [(8, 196, 3584, "bf16", 12), (8, 196, 3584, "f16", 13), (3, 576, 3584, "bf16", 14),
                              (3, 196, 1536, "bf16", 15), (4, 196, 1024, "f16", 16),
                              (2, 197, 1001, "bf16", 30)]:
        rows = mixed_rows(F, N)
        n = sel_norms(synth.make(F, N, D, DT[dn], seed, "drift"))[rows]
        lo, hi = float(n.min()), float(n.max())
        if dn == "bf16":
            out += [_case(f"B{D}-bf16-hi_out", "B", F, N, D, dn, seed, _scale(_e_above(lo, BF16_HI), rows), ["bf16_norm_above"]),
                    _case(f"B{D}-bf16-ovf", "B", F, N, D, dn, seed, _scale(_e_above(lo, 2.0 ** 64), rows), _OVF)]
        else:
            out += [_case(f"B{D}-f16-inf", "B", F, N, D, dn, seed, _scale(_e_above(lo, 65520.0), rows), ["f16_norm_over_max"]),
                    _case(f"B{D}-f16-lo_out", "B", F, N, D, dn, seed, _scale(_e_below(hi, F16_LO), rows), ["f16_norm_below"])]
    # ---- C. offset channels (massive activations): a handful of low-variance channels stay selected ------------------
    for F, N, D, dn, seed, k, v, pm in [(8, 196, 3584, "bf16", 17, 4, 2.0 ** 45, "bf16_norm_above"),
                                        (8, 196, 3584, "f16", 18, 8, 16384.0, "f16_norm_above"),
                                        (3, 576, 3584, "f16", 19, 96, 4096.0, "f16_norm_above"),
                                        (3, 196, 1536, "bf16", 20, 4, 2.0 ** 45, "bf16_norm_above")]:
        chan = low_var_channels(synth.make(F, N, D, DT[dn], seed, "drift"))
        out.append(_case(f"C{D}-{dn}-{k}x{v:g}", "C", F, N, D, dn, seed,
                         [dict(op="add", rows=None, cols=sorted(chan[:k].tolist()), value=v)], [pm]))
    # ---- D. bf16 rows of one large element and tiny others: quotients below 2^-125 (bf16-subnormal) -----------------
    # (1.5 2^30: the denominator is not a power of two, so the fast quotient x * rcp(dn) is not exact by construction)
    for F, N, D, seed, mixed in [(4, 196, 1024, 21, True), (8, 196, 3584, 22, True), (3, 196, 1536, 23, False)]:
        chan = low_var_channels(synth.make(F, N, D, torch.bfloat16, seed, "drift"))
        rows = mixed_rows(F, N) if mixed else None
        out.append(_case(f"D{D}-bf16-{'mixed' if mixed else 'all'}", "D", F, N, D, "bf16", seed,
                         _scale(-95, rows) + [dict(op="set", rows=None, cols=[int(chan[0])], value=1.5 * 2.0 ** 30)],
                         ["bf16_quot_below"]))
    # ---- E. zero rows, +-inf / NaN elements (in high-variance channels: never selected) at model width ---------------
    for F, N, D, dn, seed in [(4, 196, 1024, "bf16", 24), (4, 196, 1024, "f16", 25), (8, 196, 3584, "bf16", 26),
                              (8, 196, 3584, "f16", 27), (3, 196, 1536, "bf16", 28)]:
        var = synth.make(F, N, D, DT[dn], seed, "drift").double().var(dim=0, unbiased=False)
        hv = torch.topk(var, k=3)[1].tolist()
        out.append(_case(f"E{D}-{dn}-zero-nonfinite", "E", F, N, D, dn, seed, [
            dict(op="set", rows=mixed_rows(F, N)[:4], cols=None, value=0.0),
            dict(op="set", rows=[7, N + 9], cols=[hv[0]], value="inf"),
            dict(op="set", rows=[8], cols=[hv[1]], value="-inf"),
            dict(op="set", rows=[N + 10], cols=[hv[2]], value="nan")], ["zero"]))
    # ---- E. a corrupted token: one row inf or NaN in more than half of its channels --------------------------------
    # (those channels' variances are NaN, and torch.topk(largest=False) takes NaN variances once fewer than D / 2 are
    #  finite: selected channels that hold inf / NaN, a norm of inf / NaN, its quotients, and NaN centres from there)
    for F, N, D, dn, seed, v in [(4, 196, 1024, "bf16", 31, "nan"), (4, 196, 1024, "f16", 32, "inf"),
                                 (4, 196, 1024, "f32", 33, "nan"), (4, 196, 1024, "f32", 34, "inf"),
                                 (8, 196, 3584, "bf16", 35, "inf"), (8, 196, 3584, "f16", 36, "nan"),
                                 (8, 196, 3584, "bf16", 37, "nan"), (2, 197, 1001, "bf16", 38, "inf")]:
        out.append(_case(f"E{D}-{dn}-corrupt-{v}", "E", F, N, D, dn, seed,
                         [dict(op="set", rows=[N + 9], cols=list(range(D // 2 + 4)), value=v)], ["nonfinite"]))
    # ---- the grid mapper (LLaVA-Video: 13 x 13 tokens per frame, img_feat rows of a 13 x 14 grid) ---------------------
    F, N, D = 8, 169, 3584
    rows = mixed_rows(F, N)
    for dn, seed in (("bf16", 39), ("f16", 40)):
        n = sel_norms(synth.make(F, N, D, DT[dn], seed, "drift"))[rows]
        e, pm = (_e_above(float(n.min()), 2.0 ** 64), _OVF) if dn == "bf16" else (_e_above(float(n.min()), 65520.0),
                                                                               ["f16_norm_over_max"])
        out.append(dict(_case(f"G{D}-{dn}-llava_vid", "B", F, N, D, dn, seed, _scale(e, rows), pm), grid_h=13))
    return out


def grid_img(c) -> torch.Tensor:
    """img_feat of a grid case: [F * h * (h + 1), D] (the newline column included), as tests/golden/grid_cases.json."""
    h = c["grid_h"]
    return synth.make(c["F"], h * (h + 1), c["D"], DT[c["dtype"]], c["seed"] + 100, "iid")


# ---- scale sweeps: the whole clip by 2^e for every e of a range that crosses both window limits ----------------------
# (bf16 only: an fp16 clip cannot be scaled past either fp16 window limit with its result unchanged -- its fp16
#  variances overflow or vanish first, and the channel selection moves; families A to C cover fp16 outside the window)
SWEEPS = [dict(name="sweep-bf16", F=4, N=196, D=1024, dtype="bf16", seed=30, dist="drift", base=0.25, e_lo=-150, e_hi=100),
          dict(name="sweep-bf16-3584", F=8, N=196, D=3584, dtype="bf16", seed=32, dist="drift", base=0.25, e_lo=-150, e_hi=100)]


def sweep_input(s, e):
    return apply(synth.make(s["F"], s["N"], s["D"], DT[s["dtype"]], s["seed"], s["dist"]), _scale(e))

"""Rows built against the replay margins of the token norm, shared by tests/golden/make_margin_golden.py and
tests/test_replay_margins.py (not a conftest).

In the `torch` modes a 16-bit pass computes every token's L2 norm exactly and replays torch's own fp32 accumulation only
where the exact value lies within a margin of fp32-ulps of a T rounding boundary.  On every other fixture torch's
accumulation errs by ~10 ulps with random signs; the rows here make every rounding of torch's chains err the same way:

  fp16 (ATen's generic path: ONE sequential fp32 chain over the channels in order):  [1, 2^-5, 2^-12, 2^-12, ...].  The
      chain reaches 1 + 2^-10 after two elements, and every further s + 2^-24 is a tie that rounds to even: no small
      square ever enters the sum.  torch's norm is RN_f16(sqrt(1 + 2^-10)) = 1.0; the exact norm lies (C - 2) / 4 - 1
      fp32-ulps above the midpoint 1 + 2^-11 and rounds to 1.0009765625.
  bf16 (8 interleaved chains, element p to chain p % 8, the chains added 0..7):  one head h_j per chain, then tiny values
      t_j with t_j^2 strictly below half an ulp of h_j^2 -- each chain stays at its head's square.  The heads were found by
      a seeded random search over bf16 values in [2^-3, 2): sets whose fp32 sum of squares has a square root a few ulps
      below a bf16 midpoint, ranked by how far above it the exact norm lands (HEADS; `need` = that distance as the search
      estimated it -- the generator records the one it measures).

A case is synth.make(...) plus JSON edits (_range_inputs.apply, op "pattern").  Family S: an [F * N, C] tensor handed to
compute_gaussian_scores as already selected -- the channel order is the tensor's.  Family P: the whole pass on [F * N, D];
the heads sit in CONSTANT columns (variance 0: torch.topk sorts them first whatever their tie order -- the sums of the
heads' squares are exact in fp32, so that order does not matter), the planted rows hold one tiny value in every other
channel.  Planted rows: _range_inputs.mixed_rows (first / last row of a frame, inside a wave and a 16-row block)."""
from __future__ import annotations

import _range_inputs as RI

F16_HEAD, F16_TINY = [1.0, 2.0 ** -5], [2.0 ** -12]

# bf16 heads by C: (name suffix, heads h_0..h_7, tiny values t_0..t_7, the search's estimate of needs_ulps)
HEADS = {
    1792: [("", [1.1015625, 1.46875, 0.2080078125, 0.216796875, 0.1318359375, 0.515625, 0.2734375, 0.2041015625],
            [0.00024318695068359375, 0.0003452301025390625, 4.315376281738281e-05, 4.315376281738281e-05,
             3.039836883544922e-05, 0.00012159347534179688, 6.079673767089844e-05, 4.315376281738281e-05], 94)],
    2048: [("", [0.4609375, 1.0078125, 0.228515625, 0.2490234375, 0.205078125, 0.6171875, 0.244140625, 1.4375],
            [8.630752563476562e-05, 0.00024318695068359375, 4.315376281738281e-05, 4.315376281738281e-05,
             4.315376281738281e-05, 0.00012159347534179688, 4.315376281738281e-05, 0.0003452301025390625], 106)],
    3072: [("", [0.1484375, 1.0078125, 1.4453125, 0.1650390625, 0.37890625, 0.54296875, 0.53125, 0.1298828125],
            [3.039836883544922e-05, 0.00024318695068359375, 0.0003452301025390625, 3.039836883544922e-05,
             8.630752563476562e-05, 0.00012159347534179688, 0.00012159347534179688, 3.039836883544922e-05], 165)],
    4096: [("a", [0.431640625, 0.1337890625, 0.208984375, 1.0625, 0.29296875, 0.271484375, 0.5078125, 1.4375],
            [8.630752563476562e-05, 3.039836883544922e-05, 4.315376281738281e-05, 0.00024318695068359375,
             6.079673767089844e-05, 6.079673767089844e-05, 0.00012159347534179688, 0.0003452301025390625], 223),
           ("b", [0.71875, 0.1455078125, 0.375, 0.1328125, 0.1494140625, 0.412109375, 0.1806640625, 0.259765625],
            [0.00017261505126953125, 3.039836883544922e-05, 8.630752563476562e-05, 3.039836883544922e-05,
             3.039836883544922e-05, 8.630752563476562e-05, 4.315376281738281e-05, 6.079673767089844e-05], 220)],
}
# family P, bf16: eight heads with squares in [1, 2) and ONE tiny value for every chain (t^2 < 2^-24, half an ulp of the
# smallest square) -- exhaustive over multisets of {1 + k / 128, k < 16}: 32 ulps at C = 1792, 132 at C = 4096
P_BF16_HEADS = [1.0, 1.0078125, 1.0078125, 1.015625, 1.015625, 1.015625, 1.0234375, 1.0234375]
P_BF16_TINY = 0.00024318695068359375


def _case(name, fam, F, N, D, dn, seed, ops, rows, ratio=None):
    return dict(name=name, family=fam, F=F, N=N, D=D, dtype=dn, seed=seed, dist="drift", base=0.25, ops=ops,
                planted=len(rows), ratio=ratio)


def scored_channels(c):
    """C of a case: the tensor's width (S), int(D * ratio) of the pass (P; the reference's 0.5 unless the case has one)."""
    return c["D"] if c["family"] == "S" else int(c["D"] * (0.5 if c.get("ratio") is None else c["ratio"]))


def _p_ops(rows, D, heads, tiny):
    cols = [5 + j * (D // len(heads)) for j in range(len(heads))]                 # constant columns, spread over the row
    return [dict(op="set", rows=rows, cols=None, value=tiny)] + \
           [dict(op="set", rows=None, cols=[c], value=h) for c, h in zip(cols, heads)]


def design_cases():
    out = []
    # ---- S. compute_gaussian_scores on [F * N, C], the channel order the tensor's ---------------------------------------
    F, N = 2, 48
    rows = RI.mixed_rows(F, N)
    for i, C in enumerate((256, 384, 512, 1024, 1792, 2048, 4096)):
        out.append(_case(f"S{C}-f16", "S", F, N, C, "f16", 50 + i,
                         [dict(op="pattern", rows=rows, cols=None, head=F16_HEAD, tail=F16_TINY)], rows))
    i = 0
    for C, sets in HEADS.items():
        for suffix, heads, tiny, _ in sets:
            out.append(_case(f"S{C}{suffix}-bf16", "S", F, N, C, "bf16", 60 + i,
                             [dict(op="pattern", rows=rows, cols=None, head=heads, tail=tiny)], rows))
            i += 1
    # ---- P. the whole pass; heads in constant columns -------------------------------------------------------------------
    for i, (F, N, D) in enumerate([(4, 64, 1024), (4, 64, 2048), (4, 64, 3584), (3, 64, 4096)]):
        rows = RI.mixed_rows(F, N)
        out.append(_case(f"P{D}-f16", "P", F, N, D, "f16", 70 + i, _p_ops(rows, D, F16_HEAD, F16_TINY[0]), rows))
    for i, (F, N, D) in enumerate([(4, 64, 3584), (3, 64, 8192)]):
        rows = RI.mixed_rows(F, N)
        out.append(_case(f"P{D}-bf16", "P", F, N, D, "bf16", 80 + i, _p_ops(rows, D, P_BF16_HEADS, P_BF16_TINY), rows))
    # ... and through PassParams(channel_ratio): 3072 of 8192 channels scored
    F, N, D = 3, 64, 8192
    rows = RI.mixed_rows(F, N)
    out.append(_case(f"P{D}r-bf16", "P", F, N, D, "bf16", 82, _p_ops(rows, D, P_BF16_HEADS, P_BF16_TINY), rows, ratio=0.375))
    return out


def needs_ulps(exact_norm64, dn):
    """near_T_boundary's arithmetic on RN_f32 of the exact norms (a float64 tensor): the distance, in fp32-ulps, from
    each to the T rounding boundary (midpoint) of its T interval."""
    import torch
    drop = 16 if dn == "bf16" else 13
    bits = exact_norm64.to(torch.float32).view(torch.int32).to(torch.int64)
    return ((bits & ((1 << drop) - 1)) - (1 << (drop - 1))).abs()

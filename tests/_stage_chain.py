"""The stage chain the reference's Qwen2.5-VL / Qwen3-VL hooks call (`_compute_keep_indices`), written once for every
module that has the reference's stage API -- the reference itself (tests/golden/make_stage_chain_golden.py), vidcom2_amd on
the device (tests/test_stage_chain.py) -- plus the same chain on the CPU oracle, the inputs of the fixture's special
cases, and the digests tests/golden/stage_chain_cases.json stores -- TEST ONLY."""
import math

import torch

import oracle as O
from vidcom2_amd import synth

FP32_TOL = 1e-5          # test_gpu_parity.FP32_TOL: "similarity scores within 1e-5 fp32"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def canon(t):
    """NaNs with one bit pattern (a NaN's sign and payload are not part of the contract: NaN = NaN)."""
    t = t.detach().cpu()
    return torch.where(t.isnan(), torch.full_like(t, float("nan")), t) if t.is_floating_point() else t


def digest(t):
    return synth.sha256_tensor(canon(t))


def canon_list(t):
    """Per-frame values widened to float; NaN as the string "nan" (JSON has no NaN)."""
    return [("nan" if v != v else v) for v in t.detach().float().cpu().tolist()]


def same(a, b):
    """Bit-equal up to NaN = NaN (and -0 = +0, as torch.equal has it)."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return bool(torch.equal(a, b))
    a, b = a.double(), b.double()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def hook_chain(m, flat, frame_tokens, base_scale, ratio=None, temp=None):
    """The five calls of the hooks and the two torch expressions between them, from module `m`.  `ratio` / `temp` are the
    arguments the hooks leave at their defaults (0.5, 0.01)."""
    sel = m.select_low_var_channels(flat) if ratio is None else m.select_low_var_channels(flat, ratio)
    v, f = m.compute_gaussian_scores(sel, frame_tokens)
    s = -v.mean(dim=-1)
    scales = m.compute_scales(s, base_scale) if temp is None else m.compute_scales(s, base_scale, temp)
    total = v + f
    idx = m.select_outlier_indices(total, scales, frame_tokens)
    keep = m._map_linear_offset(idx, frame_tokens)
    return dict(sel=sel, v=v, f=f, s=s, scales=scales, total=total, idx=idx, ks=[int(i.numel()) for i in idx], keep=keep)


def oracle_chain(x, frame_tokens, base_scale, ratio=None, temp=None):
    """The same chain on the CPU oracle (in the mode it is in); its `fuse` stands for the two glue expressions."""
    order, _ = O.select_low_var_channel_idx(x, 0.5 if ratio is None else ratio)
    sel = x[:, order]
    v, f = O.compute_gaussian_scores(sel, frame_tokens)
    s, total = O.fuse(v, f)
    scales = O.compute_scales(s, base_scale, 0.01 if temp is None else temp)
    idx = O.select_outlier_indices(total, scales, frame_tokens)
    keep = O.map_linear_offset(idx, frame_tokens)
    return dict(order=order, sel=sel, v=v, f=f, s=s, scales=scales, total=total, idx=idx,
                ks=[int(i.numel()) for i in idx], keep=keep)


def case_input(c, make_input):
    """A case's input: `synth` distributions from the seed; "const" = every element 0.5 (every variance, score and
    selection a tie); "zrows" = `drift` with every seventh token of the odd frames zeroed (in fp16 the normalisation's
    eps underflows to 0: 0 / 0, NaN scores)."""
    F, N, D = c["F"], c["N"], c["D"]
    if c["dist"] == "const":
        return torch.full((F * N, D), 0.5, dtype=DT[c["dtype"]])
    if c["dist"] == "zrows":
        x = make_input(F, N, D, c["dtype"], c["seed"], "drift").clone().view(F, N, D)
        x[1::2, 3::7] = 0
        return x.view(F * N, D)
    return make_input(F, N, D, c["dtype"], c["seed"], c["dist"])


def ulps_of(dtype, got, want64):
    """max |got - want64| in units of dtype's spacing at |want64| (normal range; subnormals take the smallest normal's)."""
    mant, emin = {torch.float32: (23, -126), torch.bfloat16: (7, -126), torch.float16: (10, -14)}[dtype]
    want64 = want64.double()
    e = torch.floor(torch.log2(want64.abs().clamp(min=2.0 ** emin)))
    return float(((got.double() - want64).abs() / torch.exp2(e - mant)).max())


def fp32_margins(total, scales, ks, tpf):
    """(smallest gap between the k-th and (k+1)-th smallest total score over the frames, smallest distance of a
    scales * tpf from a half-integer): how far the reference's own fp32 numbers are from another kept set / budget."""
    gap = math.inf
    for row, k in zip(total.double(), ks):
        if k < row.numel():
            srt = row.sort().values
            gap = min(gap, float(srt[k] - srt[k - 1]))
    p = scales.double() * tpf
    half = float(((p - torch.floor(p)) - 0.5).abs().min())
    return gap, half


def check_against_golden(got, c, what="", links=None):
    """A chain's links (hook_chain's / oracle_chain's dict, `order` where it has one) against the reference's stored ones:
    16-bit bit for bit; fp32 order / sel / ks / keep exactly, scores against the stored heads within FP32_TOL (fp32
    `scales` are compared per stage, not with the golden: the softmax divides the scores' 4e-7 by temp).  links: only
    these (the oracle's `exact` mode: where the generator recorded equality)."""
    import numpy as np
    fp32 = c["dtype"] == "f32"
    on = (lambda k: True) if links is None else (lambda k: k in links)
    if "order" in got and on("order"):
        assert digest(got["order"]) == c["order_sha256"], ("channel order", what)
    if on("sel"):
        assert digest(got["sel"]) == c["sel_sha256"], ("selected features", what)
    for k in ("v", "f"):
        if fp32:
            assert np.allclose(got[k][0, :16].cpu().tolist(), c[k + "_head"], rtol=0, atol=FP32_TOL), (k, what)
        elif on(k):
            assert digest(got[k]) == c[k + "_sha256"], (k, what)
    if fp32:
        assert np.allclose(got["s"].cpu().tolist(), c["s"], rtol=0, atol=FP32_TOL), ("s", what)
    else:
        for k in ("s", "scales"):
            if on(k):
                assert canon_list(got[k]) == c[k], (k, what)
    if on("ks"):
        assert got["ks"] == c["ks"], ("budgets", what)
    if on("keep"):
        assert int(got["keep"].numel()) == c["K"] and digest(got["keep"]) == c["keep_sha256"], ("kept indices", what)

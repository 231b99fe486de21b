"""The stage chain the reference's Qwen2.5-VL / Qwen3-VL hooks call, on the device, at model widths.

Those hooks do not call `vidcom2_compression` (the fused one-launch pass nearly every other GPU test goes through): their
`_compute_keep_indices` calls select_low_var_channels -> compute_gaussian_scores -> compute_scales ->
select_outlier_indices -> _map_linear_offset with `-v.mean(dim=-1)` and `v + f` of torch's in between
(tests/_stage_chain.hook_chain).  In this library that chain runs device code the fused pass never runs: vc2_chan_var's
plan of ONE frame of R tokens, the stand-alone ORDER kernel, vc2_gather_cols, sweep 2's generic form at C = D / 2 with the
identity column order (every frame mean through margin -> flag -> replay), the stand-alone scales and selection launches,
and torch-ROCm's own `mean` and `+`.

a. the chain in `torch` mode: every link against the reference's (tests/golden/stage_chain_cases.json,
   make_stage_chain_golden.py), AND every stage against the CPU oracle on the inputs that stage actually got, so that no
   frame drops out of the comparison because an upstream value moved; the two glue expressions against the CPU's
b. the same in `torch_proven`, `exact` and debug mode 2 (replay everything)
c. the chain against the fused pass: two routes through different kernels to one result
d. vc2_chan_var alone at clip length and at row counts that are a multiple of nothing
e. arguments the hooks never pass (ratio, temp: cases of a. / b.), tpf as a tensor, map_features on the chain's indices
f. views: row slices, column slices and a storage offset that leaves the base pointer 2-byte aligned

Contract as in test_long_frames.py: 16-bit bit for bit; fp32 order / columns / budgets / kept indices exactly, scores
within 1e-6 of the oracle's `exact` mode (the kernels accumulate fp32 inputs in fp64) and FP32_TOL of the reference's."""
import ctypes

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd._ffi import check, lib

from _stage_chain import canon_list, case_input, check_against_golden, digest, hook_chain, oracle_chain, same, ulps_of
from conftest import load_json, make_input

pytestmark = pytest.mark.gpu
GOLDEN = load_json("stage_chain_cases.json")
CASES, VAR_CASES = GOLDEN["cases"], GOLDEN["var_cases"]
TARGET_RC = 128 * 196 * 1792          # rows x scored channels of the target shape: debug mode 2 is run up to here


def cid(c):
    extra = "".join(f"-{k}{c[k]:.4g}" for k in ("ratio", "temp") if c[k] is not None)
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}-{c['dtype']}-{c['dist']}-b{c['base']}{extra}"


@pytest.fixture(autouse=True)
def _default_mode():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")


@pytest.fixture(scope="module", autouse=True)
def _counters_from_zero():
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 1), "vc2_selftest_counters")     # (reset: this module's hits only)
    yield


def dev():
    return torch.device("cuda:0")


def _ratio(c):
    return 0.5 if c["ratio"] is None else c["ratio"]


def _temp(c):
    return 0.01 if c["temp"] is None else c["temp"]


_CUR = {}          # the case in hand: input (host and device) and its `torch` mode chain -- tests are ordered case by case


def _case(c):
    if _CUR.get("id") != cid(c):
        _CUR.clear()
        x = case_input(c, make_input)
        assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
        _CUR.update(id=cid(c), x=x, xd=x.to(dev()))
    return _CUR["x"], _CUR["xd"]


def _device_chain(c, xd):
    """The hook's chain from vidcom2_amd (select_outlier_indices raises on a non-zero status word), plus the channel
    order on its own; the input must come back untouched."""
    before = xd.clone()
    g = hook_chain(vc, xd, c["N"], c["base"], c["ratio"], c["temp"])
    g["order"] = vc.vidcom2.low_var_channel_order(xd, _ratio(c))
    torch.cuda.synchronize()
    assert torch.equal(xd, before), "input was modified"
    return g


def _torch_chain(c):
    x, xd = _case(c)
    if "torch" not in _CUR:
        _ffi.set_mode("torch")
        _CUR["torch"] = _device_chain(c, xd)
    return _CUR["torch"]


def _scores_close(a, b, what):
    d = (a.cpu().double() - b.cpu().double()).abs().max().item() if a.numel() else 0.0
    assert d <= 1e-6, (what, d)


def _links_same(a, b, fp32, what):
    """Two chains: every link bit-equal; fp32 scores within 1e-6, fp32 scales left to the per-stage check (the softmax
    divides the scores' differences by temp)."""
    for k in ("order", "sel", "keep"):
        assert same(a[k], b[k]), (k, what)
    assert a["ks"] == b["ks"], ("budgets", what)
    for k in ("v", "f", "s", "total") if fp32 else ("v", "f", "s", "total", "scales"):
        if fp32:
            _scores_close(a[k], b[k], (k, what))
        else:
            assert same(a[k], b[k]), (k, what)


def _check_stages(c, x, g, what):
    """Every stage against the oracle ON THE INPUT THE STAGE GOT (the oracle in the mode it is in)."""
    N, fp32 = c["N"], c["dtype"] == "f32"
    order = g["order"].cpu()
    assert torch.equal(order, O.select_low_var_channel_idx(x, _ratio(c))[0]), ("channel order", what)
    assert torch.equal(g["sel"].cpu(), x[:, order]), ("column gather", what)
    ov, of = O.compute_gaussian_scores(g["sel"].cpu(), N)
    if fp32:
        _scores_close(g["v"], ov, ("v", what)), _scores_close(g["f"], of, ("f", what))
    else:
        assert same(g["v"], ov) and same(g["f"], of), ("scores", what)
    want = O.compute_scales(g["s"].cpu(), c["base"], _temp(c))
    if fp32:
        _scores_close(g["scales"], want, ("scales", what))
    else:
        assert same(g["scales"], want), ("scales", what)
    idx = O.select_outlier_indices(g["total"].cpu(), g["scales"].cpu(), N)
    assert len(idx) == len(g["idx"]) == c["F"] and all(torch.equal(a.cpu(), b) for a, b in zip(g["idx"], idx)), \
        ("selection", what)
    assert torch.equal(g["keep"].cpu(), O.map_linear_offset([i.cpu() for i in g["idx"]], N)), ("mapping", what)


def _glue(c, g):
    """torch-ROCm's `-v.mean(dim=-1)` and `v + f` against the CPU's on the same v, f: (frames whose mean differs as
    (frame, device value, CPU value), whether the sum is bit-equal)."""
    s_dev, s_cpu = g["s"].cpu(), -g["v"].cpu().mean(dim=-1)
    ne = [(i, a, b) for i, (a, b) in enumerate(zip(canon_list(s_dev), canon_list(s_cpu))) if a != b]
    return ne, same(g["total"], g["v"].cpu() + g["f"].cpu())


# ---- a. the chain as the hook writes it ----------------------------------------------------------------------------------
def check_reference_and_per_stage(c):
    """`torch` mode.  The device's mean is expected to give the CPU's bits in every frame (on the CPU neither reversing
    the fp32 summation order nor an exact sum changed one of 1 728 bf16 / fp16 frame means; on an MI355X 0 of this
    fixture's 1 018 bf16 / fp16 frames differed): asserted, and with it every link against the reference's golden
    unconditionally.  fp32 means differ from the CPU's in the last bits (another summation order) and are held to 1e-6."""
    x, _ = _case(c)
    g = _torch_chain(c)
    mean_ne, sum_eq = _glue(c, g)
    print(f"{cid(c)}: frames whose device mean differs from the CPU's: {len(mean_ne)} of {c['F']} {mean_ne[:8]}"
          + (" (fp32: held to 1e-6, not to the bits)" if c["dtype"] == "f32" else ""))
    assert sum_eq, "v + f on the device differs from the CPU's"
    if c["dtype"] == "f32":
        _scores_close(g["s"], -g["v"].cpu().mean(dim=-1), "fp32 mean")
    else:
        assert not mean_ne, mean_ne
    check_against_golden(g, c, "torch")
    O.set_mode("exact" if c["dtype"] == "f32" else "torch")
    _check_stages(c, x, g, "torch")


# ---- b. modes ---------------------------------------------------------------------------------------------------------------
def check_torch_proven(c):
    """Proven replay margins: the `torch` mode's results and the reference's."""
    _, xd = _case(c)
    t = _torch_chain(c)
    _ffi.set_mode("torch_proven")
    g = _device_chain(c, xd)
    _links_same(g, t, c["dtype"] == "f32", "torch_proven")
    check_against_golden(g, c, "torch_proven")


def check_exact_mode(c):
    """`exact` mode against the oracle's `exact` chain link by link and stage by stage, and against the reference
    wherever the generator found the oracle's exact chain equal to it."""
    x, xd = _case(c)
    _ffi.set_mode("exact")
    O.set_mode("exact")
    g = _device_chain(c, xd)
    o = oracle_chain(x, c["N"], c["base"], c["ratio"], c["temp"])
    _links_same(g, o, c["dtype"] == "f32", "exact")
    _check_stages(c, x, g, "exact")
    rec = c["oracle"]["exact"]
    check_against_golden(g, c, "exact", links={k for k, ok in rec.items() if ok is True})


def check_replay_everything(c):
    """Debug mode 2 replays torch's order for every centre mean (fp32 inputs take no replay): `torch` mode's bits."""
    _, xd = _case(c)
    t = _torch_chain(c)
    assert lib().vc2_set_mode(2) == 0
    g = _device_chain(c, xd)
    _links_same(g, t, False, "mode 2")
    check_against_golden(g, c, "mode 2")


# ---- c. stage against fused -------------------------------------------------------------------------------------------------
def check_equals_fused_pass(c):
    """compress() -- sweep 2's streamlined / ORD forms over the column list, budgets and selection inside one launch --
    gives the chain's scores, budgets and kept indices (both ascending per frame).  The fused pass does not hand out its
    channel set, so that is compared through the scores only."""
    x, xd = _case(c)
    g = _torch_chain(c)
    got = vc.compress(xd, c["N"], c["base"], want_scores=True)
    torch.cuda.synchronize()
    if c["dtype"] == "f32":
        _scores_close(got.v_score, g["v"], "v"), _scores_close(got.f_score, g["f"], "f")
    else:
        assert same(got.v_score, g["v"]) and same(got.f_score, g["f"]), "scores"
    assert got.ks.cpu().tolist() == g["ks"] == c["ks"], "budgets"
    assert torch.equal(got.global_idx, g["keep"]) and got.K == c["K"], "kept indices"
    assert torch.equal(got.rows.cpu(), x[g["keep"].cpu()]), "rows"


# ---- d. vc2_chan_var on its own ---------------------------------------------------------------------------------------------
def check_channel_variance_alone(c):
    """One frame of R tokens (R = 100 352, 25 088, 25 087, 33): the T-rounded variance is the reference's and the oracle's
    bit for bit and `var_f32` its widening; against the fp64 variance it is allowed exactly what the reference's own
    x.var(dim=0, unbiased=False) shows on the same input (stored by the generator)."""
    x, xd = _case(c)
    var_T, var_f = vc.vidcom2._channel_variance(xd)
    torch.cuda.synchronize()
    assert digest(var_T) == c["var_sha256"]
    assert same(var_T, O.chan_var(x))
    assert torch.equal(var_f.cpu(), var_T.cpu().float())
    got = ulps_of(x.dtype, var_T.cpu(), x.double().var(dim=0, unbiased=False))
    print(f"{cid(c)}: {got:.4f} ulps from the fp64 variance (reference {c['var_ulps_vs_fp64']:.4f})")
    assert got <= c["var_ulps_vs_fp64"]


# ---- e. arguments the hook never passes -----------------------------------------------------------------------------------
def check_api_arguments(c):
    """tpf as a 1-element tensor (host or device) gives the int's scores; map_features on the chain's own index list
    gathers the kept rows; ratio / temp themselves are the `ratio` and `temp` cases of every test above."""
    x, xd = _case(c)
    g = _torch_chain(c)
    for tpf in (torch.tensor([c["N"]]), torch.tensor(c["N"], device=dev())):
        v, f = vc.compute_gaussian_scores(g["sel"], tpf)
        assert torch.equal(v, g["v"]) and torch.equal(f, g["f"])
    rows = vc.map_features(g["idx"], xd, None, vc.MODEL_SPECS["qwen2_5_vl"])
    assert torch.equal(rows.cpu(), x[g["keep"].cpu()])
    assert synth.sha256_tensor(vc._map_linear_offset([i.clone() for i in g["idx"]], torch.tensor(c["N"])).cpu()) \
        == c["keep_sha256"]


# ---- the checks, case by case ------------------------------------------------------------------------------------------------
def _checks_of(c):
    """Which checks a case takes, decided here at collection (nothing is left out at run time): debug mode 2 for 16-bit
    cases up to the target's rows x scored channels, the fused pass where the hook's defaults hold, the variance alone for
    the clip-length cases, the API arguments on the ratio / temp / scalar cases and a few plain ones."""
    out = ["reference_and_per_stage", "torch_proven", "exact_mode"]
    if c["dtype"] != "f32" and c["F"] * c["N"] * int(c["D"] * _ratio(c)) <= TARGET_RC:
        out.append("replay_everything")
    if c["ratio"] is None and c["temp"] is None:
        out.append("equals_fused_pass")
    if c["var"]:
        out.append("channel_variance_alone")
    if c["name"] in ("ratio", "temp", "scalar", "one_token", "w1536", "f32"):
        out.append("api_arguments")
    return out


@pytest.mark.parametrize("c,what", [(c, w) for c in CASES for w in _checks_of(c)], ids=lambda v: v if isinstance(v, str) else cid(v))
def test_chain(c, what):
    """Every check of one case in a row (the input is generated and uploaded once): see check_<what>."""
    globals()["check_" + what](c)


@pytest.mark.parametrize("c", VAR_CASES, ids=cid)
def test_channel_variance_alone(c):
    check_channel_variance_alone(c)


# ---- f. views -----------------------------------------------------------------------------------------------------------------
def _views(x):
    """(name, the buffer, the view of it that equals x)."""
    R, D = x.shape
    rows = torch.zeros(R + 2, D, dtype=x.dtype, device=x.device)
    rows[1:R + 1] = x
    wide = torch.zeros(R, D + 24, dtype=x.dtype, device=x.device)
    wide[:, :D] = x
    flat = torch.zeros(R * D + 8, dtype=x.dtype, device=x.device)
    flat[3:3 + R * D] = x.reshape(-1)
    return [("rows", rows, rows[1:R + 1]), ("columns", wide, wide[:, :D]), ("offset", flat, flat[3:3 + R * D].view(R, D))]


@pytest.mark.parametrize("shape", [(4, 100, 3584), (5, 169, 1001)], ids=lambda s_: "x".join(map(str, s_)))
def test_views_of_larger_tensors(shape):
    """The hooks hand over slices of larger tensors.  A row slice, a column slice (not contiguous) and a storage offset
    of 3 elements -- at D = 1001 a row is 2002 bytes, so the row slice starts 2-byte aligned as well -- through the chain
    and through compress(): the clone's results bit for bit, the buffer untouched.  (include/vc2.h asks for 16-byte
    aligned base pointers: the wrappers copy a view that is not.)"""
    F, N, D = shape
    xd = make_input(F, N, D, "bf16", 170, "drift").to(dev())
    want = hook_chain(vc, xd.clone(), N, 0.25)
    want["order"] = vc.vidcom2.low_var_channel_order(xd.clone())
    fused = vc.compress(xd.clone(), N, 0.25, want_scores=True)
    for name, buf, view in _views(xd):
        assert torch.equal(view, xd) and (name == "columns") != view.is_contiguous()
        before = buf.clone()
        g = hook_chain(vc, view, N, 0.25)
        g["order"] = vc.vidcom2.low_var_channel_order(view)
        _links_same(g, want, False, name)
        got = vc.compress(view, N, 0.25, want_scores=True)
        torch.cuda.synchronize()
        assert torch.equal(got.v_score, fused.v_score) and torch.equal(got.f_score, fused.f_score), name
        assert torch.equal(got.ks, fused.ks) and torch.equal(got.global_idx, fused.global_idx), name
        assert torch.equal(got.rows, fused.rows) and torch.equal(got.rows, xd[got.global_idx]), name
        assert torch.equal(buf, before), (name, "the buffer was modified")
        # the later stages on views of their own inputs
        pad = torch.zeros(F + 2, N, dtype=xd.dtype, device=dev())
        pad[1:F + 1] = want["total"]
        idx = vc.select_outlier_indices(pad[1:F + 1], want["scales"], N)
        assert all(torch.equal(a, b) for a, b in zip(idx, want["idx"])), name


# ---- the module's last test -------------------------------------------------------------------------------------------------
def test_no_selection_loop_bound_expired():
    """After everything above: no bounded loop of the selection replay (channel selection, ORDER kernel, per-frame
    selection) ever ran into its bound."""
    _CUR.clear()
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)

"""LLaVA-Video's grid pass (mapper "grid_vid") against the CPU oracle.

This is the one pass that does more than pick rows of its input.  The selection kernel (select_frame_body) maps each
kept token p of frame f onto the h x (h + 1) newline grid, f*h*(h+1) + (p/h)*(h+1) + p%h.  It writes the frame's h
newline rows behind its kept tokens and puts grid_h extra slots into every frame's output offset (k_select's budget
prologue).  CompressPlan adds F * grid_h to the capacity, and the gather reads img_feat [F*h*(h+1), D], not the scored
tensor.  K counts the newline rows; ks does not.

The expected result is built from the oracle: compress_indices on the scored tensor, its local indices per frame,
map_grid_vid, then img[...].  For h = 13 that also equals the oracle's vidcom2_compression(model="llava_vid").  The
contract is test_full_pass's: budgets and mapped indices exact, rows bit-equal to img[global_idx], half-precision scores
bit-equal to the oracle in the same mode, fp32 scores within 1e-6 of the oracle's `exact` mode (the kernels accumulate
fp32 inputs in fp64 in either mode, DESIGN.md "Numerics contract").

Budgets are clamped to k >= 1 (vidcom2.py:72), so no frame of a pass keeps nothing but its newline rows.  The lowest
budgets come from base 0.005 and 0.01 (k = 1 to 3 of 169).  Frames that are only newline rows are reached through the
stage API (_map_grid_vid on lists with empty frames)."""
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd.vidcom2 import MODEL_SPECS, CompressPlan

from conftest import DT, load_json, make_input

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_mode():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")


def dev():
    return torch.device("cuda:0")


def nan_eq(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _set_modes(mode, dn):
    """GPU in `mode`; the oracle in `mode` for half precision, in `exact` for fp32 (see the module docstring)."""
    _ffi.set_mode(mode)
    O.set_mode(mode if dn != "f32" else "exact")


def _img(F, h, D, dn, seed):
    """A stand-in for add_token_per_grid's output: [F * h * (h + 1), D], newline column included."""
    return synth.make(F, h * (h + 1), D, DT[dn], seed, "iid")


def _grid_ref(x, h, base, img):
    """The oracle's grid pass: compress_indices, local indices per frame, map_grid_vid, img[...]."""
    N = h * h
    F = x.shape[0] // N
    o = O.compress_indices(x, N, base)
    loc = o["global_idx"] - torch.repeat_interleave(torch.arange(F) * N, o["ks"])
    g = O.map_grid_vid(list(torch.split(loc, o["ks"].tolist())), h)
    o["grid_idx"] = g
    if h == 13:
        assert torch.equal(O.vidcom2_compression(x, model="llava_vid", base_scale=base, img_feat=img), img[g])
    return o


def _check_grid(got, ref, img, h, dn, what=""):
    F = ref["ks"].numel()
    ks = got.ks.cpu()
    assert ks.tolist() == ref["ks"].tolist(), ("budgets", what)
    assert got.K == int(ks.sum()) + F * h, ("K counts the newline rows", what)
    gi = got.global_idx.cpu()
    assert torch.equal(gi, ref["grid_idx"]), ("mapped indices", what)
    if got.v_score is not None:
        if dn == "f32":
            assert (got.v_score.cpu() - ref["v"]).abs().max().item() <= 1e-6, ("v_score", what)
            assert (got.f_score.cpu() - ref["f"]).abs().max().item() <= 1e-6, ("f_score", what)
        else:
            assert nan_eq(got.v_score, ref["v"]) and nan_eq(got.f_score, ref["f"]), ("scores", what)
    if got.rows is not None:
        assert got.rows.shape == (got.K, img.shape[1]), ("rows shape", what)
        assert torch.equal(got.rows.cpu(), img.cpu()[gi]), ("rows", what)


def _run(x, h, base, img, mode, dn, **kw):
    """HIP and the oracle on one clip; the inputs must come back unmodified."""
    _set_modes(mode, dn)
    ref = _grid_ref(x, h, base, img)
    xd, imgd = x.to(dev()), img.to(dev())
    got = vc.compress(xd, h * h, base, "grid_vid", h, imgd, want_scores=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x) and torch.equal(imgd.cpu(), img), "an input was modified"
    _check_grid(got, ref, img, h, dn)
    return got, ref


# ---- the reference's own vectors (tests/golden/grid_cases.json) --------------------------------------------------
@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("c", load_json("grid_cases.json")["cases"], ids=lambda c: f"{c['name']}-{c['dtype']}")
def test_reference_grid_cases(c, mode):
    """HIP == the oracle in the same mode, and == the reference's budgets, mapped indices and rows (every case is
    index-exact between oracle and reference in both modes, see test_oracle_golden.test_grid_pass_vs_reference)."""
    h, F = c["h"], c["F"]
    x = make_input(F, c["N"], c["D"], c["dtype"], c["seed"], c["dist"])
    img = synth.make(F, h * (h + 1), c["D"], DT[c["dtype"]], c["img_seed"], "iid")
    assert synth.sha256_tensor(x) == c["x_sha256"] and synth.sha256_tensor(img) == c["img_sha256"]
    got, _ = _run(x, h, c["base"], img, mode, c["dtype"])
    assert got.ks.cpu().tolist() == c["ks"] and got.K == c["K"]
    assert synth.sha256_tensor(got.global_idx) == c["idx_sha256"]
    assert synth.sha256_tensor(got.rows) == c["out_sha256"]
    if c["h"] == MODEL_SPECS["llava_vid"]["grid"]:
        out = vc.vidcom2_compression(x.to(dev()), model="llava_vid", base_scale=c["base"], img_feat=img.to(dev()))
        assert synth.sha256_tensor(out) == c["out_sha256"]


# ---- the model's shapes: h = 13, D = 3584 (LLaVA-Video-7B) and 5120 (16-bit D > 4096 row path) -------------------
MODEL_CASES = [(F, 3584, dn) for F in (1, 16, 64) for dn in ("f32", "bf16", "f16")] + [(16, 5120, "bf16"),
                                                                                        (9, 5120, "f16")]


@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_model_shapes(case, mode):
    F, D, dn = case
    x = make_input(F, 169, D, dn, 5, "drift")
    _run(x, 13, 0.15, _img(F, 13, D, dn, 6), mode, dn)


# ---- every branch of the selection engine under grid mapping ------------------------------------------------------
# select_frame_body picks its engine by N = h * h and the word size (32-bit words for 16-bit inputs, 64-bit for fp32):
#   16-bit: N <= 256 -> topk_smallest4_solo<4>   (h = 1, 2, 7, 16)
#           N <= 512 -> topk_smallest4_solo<8>   (h = 22: 484)
#           N <= 1020 = sel2_capacity(1, 4) -> one-wave topk_smallest2<1, 4, 4>   (h = 23: 529, h = 31: 961)
#           N > 1020 -> four-wave topk_smallest2<4, 4, 8>   (h = 32: 1024, h = 45: 2025)
#   fp32:   N <= 1020 -> one-wave topk_smallest2 (h <= 31), N > 1020 -> four waves (h = 32, 45)
ENGINE_H = [1, 2, 7, 16, 22, 23, 31, 32, 45]


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("h", ENGINE_H)
def test_engine_classes(h, dn):
    F = 6
    x = make_input(F, h * h, 128, dn, 11, "drift")
    _run(x, h, 0.25, _img(F, h, 128, dn, 12), "torch", dn)


# ---- budget extremes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("base", [0.005, 0.01, 0.9, 1.0])
def test_budget_extremes(base, dn):
    """base 0.005 / 0.01: k = 1 to 3 per frame, the frame is mostly newline rows; base 0.9 / 1.0: scales clamp at 1,
    whole frames (k = N) are kept, and a frame's newline rows sit right behind all of its h * h tokens."""
    F, h = 12, 13
    x = make_input(F, h * h, 256, dn, 21, "drift")
    got, ref = _run(x, h, base, _img(F, h, 256, dn, 22), "torch", dn)
    ks = ref["ks"]
    if base < 0.1:
        assert int(ks.max()) <= 3 and (base > 0.005 or int(ks.min()) == 1)
    else:
        assert int(ks.max()) == h * h


@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("base", [0.01, 0.25, 1.0])
def test_constant_input(base, dn):
    """Every score ties: pure tie-breaking, and every frame gets the same budget (1 .. N)."""
    F, h = 5, 13
    x = torch.full((F * h * h, 64), 0.5, dtype=DT[dn])
    got, ref = _run(x, h, base, _img(F, h, 64, dn, 23), "torch", dn)
    assert len(set(ref["ks"].tolist())) == 1
    if base == 1.0:
        assert ref["ks"].tolist() == [h * h] * F


# ---- more than 1024 frames: budgets from scales_f32, the other offset loop of k_select -------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_many_frames(dn):
    F, h = 1100, 13
    x = make_input(F, h * h, 64, dn, 31, "drift")
    _run(x, h, 0.25, _img(F, h, 64, dn, 32), "torch", dn)


# ---- img_feat ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_img_feat_layouts(dn):
    """Exactly F*h*(h+1) rows; more rows than needed, whose extra rows (a poison value) never reach `rows`; a
    non-contiguous img_feat (every other column of a wider tensor) and one that starts at a storage offset."""
    F, h, D = 4, 13, 128
    x = make_input(F, h * h, D, dn, 41, "drift")
    img = _img(F, h, D, dn, 42)
    _run(x, h, 0.25, img, "torch", dn)
    longer = torch.cat((img, torch.full((37, D), 4096.0, dtype=DT[dn])))
    got, _ = _run(x, h, 0.25, longer, "torch", dn)
    assert not (got.rows == 4096.0).all(dim=1).any()
    wide = torch.stack((img, -img), dim=2).reshape(img.shape[0], 2 * D)      # img in the even columns
    strided = wide.to(dev())[:, 0::2]
    assert not strided.is_contiguous()
    got = vc.compress(x.to(dev()), h * h, 0.25, "grid_vid", h, strided)
    _check_grid(got, _grid_ref(x, h, 0.25, img), img, h, dn, "strided img_feat")
    offset = torch.cat((torch.zeros(5, D, dtype=DT[dn]), img)).to(dev())[5:]
    got = vc.compress(x.to(dev()), h * h, 0.25, "grid_vid", h, offset)
    _check_grid(got, _grid_ref(x, h, 0.25, img), img, h, dn, "img_feat at a storage offset")


# ---- call options --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_options(dn):
    F, h, D = 8, 13, 256
    _set_modes("torch", dn)
    x = make_input(F, h * h, D, dn, 51, "drift")
    img = _img(F, h, D, dn, 52)
    ref = _grid_ref(x, h, 0.25, img)
    xd, imgd = x.to(dev()), img.to(dev())
    a = vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, gather=False)            # indices only
    assert a.rows is None
    _check_grid(a, ref, img, h, dn, "gather=False")
    b = vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, want_scores=False)
    c = vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, want_scores=True)
    assert b.v_score is None and c.v_score is not None
    assert torch.equal(b.global_idx, c.global_idx) and torch.equal(b.ks, c.ks) and torch.equal(b.rows, c.rows)
    _check_grid(b, ref, img, h, dn, "want_scores=False")
    _check_grid(c, ref, img, h, dn, "want_scores=True")


@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_two_clips_through_one_plan(dn):
    """Two clips of different content and budgets on one shape: through the one-shot API (its cached plan), and
    through one CompressPlan whose output tensors are re-used.  The second clip's newline slots and rows are its own:
    nothing of the first clip's survives in them."""
    F, h, D = 6, 13, 128
    _set_modes("torch", dn)
    xa, xb = make_input(F, h * h, D, dn, 61, "drift"), make_input(F, h * h, D, dn, 62, "iid")
    ia, ib = _img(F, h, D, dn, 63), -_img(F, h, D, dn, 64) - 3
    ra, rb = _grid_ref(xa, h, 0.25, ia), _grid_ref(xb, h, 0.25, ib)
    assert ra["ks"].tolist() != rb["ks"].tolist()                    # the newline slots move between the clips
    for _ in range(2):
        _check_grid(vc.compress(xa.to(dev()), h * h, 0.25, "grid_vid", h, ia.to(dev())), ra, ia, h, dn, "clip a")
        _check_grid(vc.compress(xb.to(dev()), h * h, 0.25, "grid_vid", h, ib.to(dev())), rb, ib, h, dn, "clip b")
    plan = CompressPlan(F, h * h, D, DT[dn], dev(), 0.25, "grid_vid", h)
    assert plan.cap >= max(ra["grid_idx"].numel(), rb["grid_idx"].numel())
    plan.idx.fill_(-7)
    plan.rows.fill_(float("nan"))
    for x, img, ref in ((xa, ia, ra), (xb, ib, rb), (xa, ia, ra)):
        plan.enqueue(x.to(dev()), img.to(dev()))
        got = plan.finish()
        _check_grid(got, ref, img, h, dn, "re-used plan outputs")


# ---- fused pooling: pool_stats -> compress(..., "grid_vid", stats_ws=...) -----------------------------------------
POOL_CASES = [("average", 26), ("average", 27), ("max", 26), ("max", 27), ("bilinear", 25), ("bilinear", 26)]


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
@pytest.mark.parametrize("mode,H", POOL_CASES, ids=lambda v: str(v))
def test_fused_pooling(mode, H, dn):
    """What the LLaVA grid hook does on every GPU call: get_2dPool fused with sweep 1 (a 13 x 13 grid), the newline
    column appended as add_token_per_grid does, then the grid pass on the statistics pool_stats left."""
    from test_fused import _torch_pool
    from vidcom2_amd.fused import pool_stats
    F, D, h = 5, 128, 13
    _set_modes("torch", dn)
    g = torch.Generator().manual_seed(H * 7 + len(mode))
    feat = torch.randn(F, H * H, D, generator=g).to(DT[dn])
    newline = torch.randn(D, generator=g).to(DT[dn])
    out, ws = pool_stats(feat.to(dev()), H, H, mode)
    pooled = out.cpu()
    it = torch.int32 if dn == "f32" else torch.int16
    assert out.shape == (F, h * h, D) and torch.equal(pooled.view(it), _torch_pool(feat, H, H, mode).view(it))
    img = torch.cat((out.reshape(F, h, h, D), newline.to(dev()).expand(F, h, 1, D)), dim=2).reshape(F * h * (h + 1), D)
    flat = out.reshape(-1, D)
    assert ws._vc2_stats_for == (F, h * h, D, DT[dn], flat.data_ptr())       # the pass does take the fused statistics
    got = vc.compress(flat, h * h, 0.25, "grid_vid", h, img, want_scores=True, stats_ws=ws)
    img_cpu = img.cpu()
    _check_grid(got, _grid_ref(pooled.reshape(-1, D), h, 0.25, img_cpu), img_cpu, h, dn, (mode, H))
    assert torch.equal(got.rows.cpu()[-h:], newline.expand(h, D))             # the last frame's newline rows


# ---- the stage API -----------------------------------------------------------------------------------------------
def test_stage_api_matches_the_oracle():
    """select_outlier_indices -> _map_grid_vid -> map_features(..., MODEL_SPECS["llava_vid"]) at 16 x 169 x 3584,
    the reference's own sequence of calls (vidcom2.py:27-36)."""
    F, N, D, base = 16, 169, 3584, 0.15
    x = make_input(F, N, D, "bf16", 71, "drift")
    img = _img(F, 13, D, "bf16", 72)
    ref = _grid_ref(x, 13, base, img)
    xd, imgd = x.to(dev()), img.to(dev())
    v, f = vc.compute_gaussian_scores(vc.select_low_var_channels(xd), N)
    assert torch.equal(v.cpu(), ref["v"]) and torch.equal(f.cpu(), ref["f"])
    scales = vc.compute_scales((-v.cpu().mean(dim=-1)).to(dev()), base)       # (the frame means as the CPU takes them)
    ind = vc.select_outlier_indices(v + f, scales, N)
    assert [int(i.numel()) for i in ind] == ref["ks"].tolist()
    assert torch.equal(vc._map_grid_vid(ind, 13).cpu(), ref["grid_idx"])
    rows = vc.map_features(ind, xd, imgd, MODEL_SPECS["llava_vid"])
    assert torch.equal(rows.cpu(), img[ref["grid_idx"]])


@pytest.mark.parametrize("h", [1, 13, 32])
def test_map_grid_vid_with_empty_frames(h):
    """_map_grid_vid == the oracle's map_grid_vid on index lists with empty frames (only the newline rows), full
    frames and single tokens (k_map_indices)."""
    g = torch.Generator().manual_seed(h)
    N = h * h
    sizes = [0, N, 1, 0, max(1, N // 3), 0, N // 2]
    ind = [torch.randperm(N, generator=g)[:k].sort().values for k in sizes]
    want = O.map_grid_vid(ind, h)
    assert want.numel() == sum(sizes) + len(sizes) * h
    got = vc._map_grid_vid([i.to(dev()) for i in ind], h)
    assert torch.equal(got.cpu(), want)


# ---- errors, and the next valid call after each ------------------------------------------------------------------
def test_errors_leave_the_next_call_right():
    F, h, D, dn = 4, 13, 128, "bf16"
    x = make_input(F, h * h, D, dn, 81, "drift")
    img = _img(F, h, D, dn, 82)
    ref = _grid_ref(x, h, 0.25, img)
    xd, imgd = x.to(dev()), img.to(dev())

    def valid():
        _check_grid(vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, want_scores=True), ref, img, h, dn, "after")

    valid()
    for bad_h in (12, 0, -13):                           # N != h^2 and grid_h <= 0: the C argument check
        with pytest.raises(RuntimeError, match="grid_vid mapping needs N == grid_h"):
            vc.compress(xd, h * h, 0.25, "grid_vid", bad_h, imgd)
        valid()
    for bad in (imgd.float(), imgd[:, : D - 8].contiguous()):      # another dtype, another width
        with pytest.raises(RuntimeError, match="img_feat must have the dtype and feature dim"):
            vc.compress(xd, h * h, 0.25, "grid_vid", h, bad)
        valid()
    with pytest.raises(IndexError):                       # one row short
        vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd[:-1])
    valid()

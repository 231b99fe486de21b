"""GPU: `compress(x, ..., score_dtype=torch.float32)` on bf16 / fp16 tensors -- the reference applied to x.float(), from
the 16-bit tensor itself.  The contract (DESIGN.md "Scoring 16-bit features in fp32"): budgets and kept indices equal
the reference's (tests/golden/score_dtype_cases.json, whose cases keep every decision 5e-6 apart) and the CPU oracle's on
the widened input, scores within 1e-6 of the oracle's and 1e-5 of the reference's recorded values, rows = x[global_idx]
bit for bit in x's dtype."""
import hashlib
import os
import types

import numpy as np
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth

import _score_dtype as SD
import _stub_models as S
from conftest import load_core_cases, make_input

pytestmark = pytest.mark.gpu

CASES = SD.load()
F32 = torch.float32


@pytest.fixture(autouse=True)
def _modes():
    O.set_mode("exact")
    _ffi.set_mode("torch")
    yield
    O.set_mode("torch")
    _ffi.set_mode("torch")


def _params(c):
    if not SD.has_params(c):
        return None
    kw = {}
    if c["ratio"] is not None:
        kw["channel_ratio"] = c["ratio"]
    if c["temp"] is not None:
        kw["temp"] = c["temp"]
    if c["alphas"] is not None:
        kw["alphas"] = c["alphas"]
    return vc.PassParams(**kw)


def _first(F, N, D, dtype, **kw):
    for c in CASES:
        if (c["F"], c["N"], c["D"], c["dtype"]) == (F, N, D, dtype) and c["mapper"] == "linear" and not SD.has_params(c) \
                and c["base"] == 0.25 and all(c[k] == v for k, v in kw.items()):
            return c
    raise AssertionError(f"no fixture {F}x{N}x{D} {dtype} {kw}")


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


# ---- 1. parity, per fixture ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=SD.case_id)
def test_parity_with_the_reference_on_the_widened_input(c):
    x = SD.make_input(c)
    xg = x.cuda()
    before = xg.clone()
    kw = {}
    src = x
    if c["mapper"] == "grid_vid":
        src = SD.make_img(c)
        kw = dict(mapper="grid_vid", grid_h=SD.grid_h(c), img_feat=src.cuda())
    got = vc.compress(xg, c["N"], c["base"], want_scores=True, score_dtype=F32, params=_params(c), **kw)
    torch.cuda.synchronize()
    assert torch.equal(xg, before), "the input was modified"
    ks, gidx = got.ks.cpu().tolist(), got.global_idx.cpu()
    assert ks == c["ks"]
    assert gidx.tolist() == c["global_idx"] and got.K == c["K"]
    assert got.rows.dtype == x.dtype and torch.equal(got.rows.cpu(), src[gidx])
    assert got.v_score.dtype == F32 and got.f_score.dtype == F32
    v, f = got.v_score.cpu(), got.f_score.cpu()
    dv = np.abs(np.asarray(v[0, :16].tolist()) - np.asarray(c["v_head"])).max()
    df = np.abs(np.asarray(f[0, :16].tolist()) - np.asarray(c["f_head"])).max()
    print(SD.case_id(c), "max |d| from the recorded heads: v", dv, "f", df)
    assert dv <= SD.HEAD_TOL and df <= SD.HEAD_TOL
    if not SD.has_params(c):               # (the oracle's whole-pass call has no params: those cases stand on the fixture)
        ref = O.compress_indices(x.float(), c["N"], c["base"])
        assert ks == ref["ks"].tolist()
        lin = ref["global_idx"]
        want = SD.grid_indices(lin, ks, c) if c["mapper"] == "grid_vid" else lin
        assert torch.equal(gidx, want)
        ev = float((v.double() - ref["v"].double()).abs().max())
        ef = float((f.double() - ref["f"].double()).abs().max())
        print(SD.case_id(c), "max |d| from the oracle: v", ev, "f", ef)
        assert ev <= SD.SCORE_TOL and ef <= SD.SCORE_TOL


# ---- 2. against the project's own fp32-input pass -----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(4, 49, 64, "bf16"), (3, 50, 100, "f16"), (2, 196, 3584, "bf16")],
                         ids=["vector", "scalar", "model-width"])
def test_same_result_as_the_fp32_pass_on_the_widened_tensor(shape):
    c = _first(*shape)
    xg = SD.make_input(c).cuda()
    a = vc.compress(xg, c["N"], c["base"], want_scores=True, score_dtype=F32)
    b = vc.compress(xg.float(), c["N"], c["base"], want_scores=True)
    assert a.ks.tolist() == b.ks.tolist() and torch.equal(a.global_idx, b.global_idx)
    assert float((a.v_score - b.v_score).abs().max()) <= SD.SCORE_TOL
    assert float((a.f_score - b.f_score).abs().max()) <= SD.SCORE_TOL
    assert a.rows.dtype == xg.dtype and b.rows.dtype == F32 and torch.equal(a.rows.float(), b.rows)


# ---- 3. the no-op forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_none_and_the_input_dtype_are_the_plain_call(dt):
    c = min((c for c in load_core_cases() if c["dtype"] == dt), key=lambda c: c["F"] * c["N"] * c["D"])
    x = make_input(c["F"], c["N"], c["D"], dt, c["seed"], c["dist"]).cuda()
    base = c.get("base", 0.25)
    cache = vc.vidcom2._PLAN_CACHE
    vc.vidcom2.clear_plan_cache()
    plain = vc.compress(x, c["N"], base, want_scores=True)
    keys = list(cache)
    assert len(keys) == 1
    for sd in (None, x.dtype):
        r = vc.compress(x, c["N"], base, want_scores=True, score_dtype=sd)
        assert list(cache) == keys, "a no-op score_dtype made a plan of its own"
        assert torch.equal(r.global_idx, plain.global_idx) and torch.equal(r.ks, plain.ks)
        assert r.rows.dtype == x.dtype and _sha(r.rows) == _sha(plain.rows)
        assert r.v_score.dtype == x.dtype
        assert _sha(r.v_score) == _sha(plain.v_score) and _sha(r.f_score) == _sha(plain.f_score)
    if dt == "bf16":
        with pytest.raises(ValueError, match="score_dtype"):
            vc.compress(x, c["N"], base, score_dtype=torch.float16)
        with pytest.raises(ValueError, match="score_dtype"):
            vc.compress_batch([x, x], c["N"], base, score_dtype=torch.float16)
        assert list(cache) == keys, "a refused call touched the plan cache"


# ---- 4. options --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smoke_shape():
    c = _first(8, 196, 1024, "bf16")
    x = SD.make_input(c).cuda()
    return c, x, vc.compress(x, c["N"], c["base"], want_scores=True, score_dtype=F32)


def test_gather_false(smoke_shape):
    c, x, full = smoke_shape
    r = vc.compress(x, c["N"], c["base"], gather=False, score_dtype=F32)
    assert r.rows is None and torch.equal(r.global_idx, full.global_idx) and torch.equal(r.ks, full.ks)


def test_tail_row(smoke_shape):
    c, x, full = smoke_shape
    tail = synth.make(1, 1, c["D"], x.dtype, 99, "iid").cuda()
    r = vc.compress(x, c["N"], c["base"], tail=tail, score_dtype=F32)
    assert r.rows.shape == (full.K + 1, c["D"]) and r.rows.dtype == x.dtype
    assert torch.equal(r.rows[:-1], full.rows) and torch.equal(r.rows[-1:], tail)


def test_without_scores(smoke_shape):
    c, x, full = smoke_shape
    r = vc.compress(x, c["N"], c["base"], want_scores=False, score_dtype=F32)
    assert r.v_score is None and r.f_score is None
    assert torch.equal(r.global_idx, full.global_idx) and torch.equal(r.rows, full.rows)


def test_pool_stats_workspace():
    from vidcom2_amd.fused import pool_stats
    F, H, D = 8, 27, 1024
    xin = synth.make(F, H * H, D, torch.bfloat16, 7, "drift").cuda().view(F, H * H, D)
    pooled, ws = pool_stats(xin, H, H, "average")
    n = pooled.shape[1]
    assert n == 13 * 13
    flat = pooled.view(F * n, D)
    a = vc.compress(flat, n, 0.25, want_scores=True, stats_ws=ws, score_dtype=F32)
    b = vc.compress(flat.clone(), n, 0.25, want_scores=True, score_dtype=F32)       # (a copy: sweep 1 runs)
    assert a.v_score.dtype == F32
    assert torch.equal(a.ks, b.ks) and torch.equal(a.global_idx, b.global_idx) and torch.equal(a.rows, b.rows)
    assert torch.equal(a.v_score, b.v_score) and torch.equal(a.f_score, b.f_score)
    ref = O.compress_indices(flat.cpu().float(), n, 0.25)
    assert a.ks.tolist() == ref["ks"].tolist()


def test_batch_of_three_equals_three_calls():
    cs = [c for c in CASES if (c["F"], c["N"], c["D"], c["dtype"]) == (8, 196, 1024, "bf16") and not SD.has_params(c)][:3]
    assert len(cs) == 3
    clips = [SD.make_input(c).cuda() for c in cs]
    got = vc.compress_batch(clips, 196, 0.25, score_dtype=F32)
    for c, x, r in zip(cs, clips, got):
        one = vc.compress(x, 196, 0.25, score_dtype=F32)
        assert r.ks.tolist() == one.ks.tolist() == c["ks"]
        assert torch.equal(r.global_idx, one.global_idx) and r.global_idx.tolist() == c["global_idx"]
        assert r.rows.dtype == x.dtype and torch.equal(r.rows, one.rows)


def test_numerics_mode_changes_nothing(smoke_shape):
    c, x, full = smoke_shape
    _ffi.set_mode("exact")
    try:
        r = vc.compress(x, c["N"], c["base"], want_scores=True, score_dtype=F32)
    finally:
        _ffi.set_mode("torch")
    assert torch.equal(r.global_idx, full.global_idx) and torch.equal(r.ks, full.ks) and torch.equal(r.rows, full.rows)
    assert torch.equal(r.v_score, full.v_score) and torch.equal(r.f_score, full.f_score)


# ---- 5. autograd -------------------------------------------------------------------------------------------------
def test_rows_backpropagate_like_an_index():
    c = _first(4, 49, 64, "bf16")
    x = SD.make_input(c).cuda().requires_grad_()
    r = vc.compress(x, c["N"], c["base"], score_dtype=F32)
    assert r.global_idx.tolist() == c["global_idx"]
    r.rows.sum().backward()
    x2 = x.detach().clone().requires_grad_()
    x2[r.global_idx].sum().backward()
    assert x.grad.dtype == x.dtype and torch.equal(x.grad, x2.grad)


# ---- 6. the hooks' knob -------------------------------------------------------------------------------------------
def test_qwen25_hook_scores_in_fp32_when_the_knob_says_so(monkeypatch):
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    c = dict(D=128, dt="bf16", seed=21, r="0.25", grids=[[8, 12, 12]], prefix=15, between=0, suffix=9, mask="2d")
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", c["r"])
    monkeypatch.setenv("VC2_SCORE_DTYPE", "fp32")
    ids, feats, pos, mask = S.qwen_inputs(c)
    model, rec = S.make_qwen_vl_model("qwen2_5_vl", c["D"], torch.bfloat16, "cuda", c["seed"])
    S.set_video_features(model, [f.cuda() for f in feats])
    model.forward = types.MethodType(hook, model)
    model(input_ids=ids.cuda(), attention_mask=mask.cuda(), position_ids=pos.cuda(),
          pixel_values_videos=torch.zeros(1, 4, device="cuda"), video_grid_thw=torch.tensor(c["grids"], device="cuda"))
    seen = rec.calls[-1]["position_ids"][0, 0].tolist()
    tpf = (12 * 12) // 4
    embeds = feats[0].cuda()
    keep = vc.compress(embeds, tpf, 0.25, gather=False, score_dtype=F32).global_idx.tolist()
    n_video = embeds.shape[0]
    want = list(range(c["prefix"])) + [c["prefix"] + i for i in keep] + \
        [c["prefix"] + n_video + j for j in range(c["suffix"])]
    assert seen == want

"""The one-launch pass with non-default hyper-parameters (`compress(..., params=PassParams(...))`, vc2_compress_ex3) on
the device.

1. parity with the REFERENCE: every ratio / temp case of tests/golden/stage_chain_cases.json and every case of
   tests/golden/pass_params_cases.json (make_pass_params_golden.py) through the fused pass in `torch` mode -- 16-bit: both
   scores, budgets, K, kept indices and rows bit for bit; fp32: budgets and kept indices exactly, scores within FP32_TOL
2. the fused pass against the stage-by-stage route (other kernels) on fresh seeds, `torch` and `exact` modes
3. a PassParams equal to the defaults IS the default pass: bits, cached plan, kernels
4. compress_batch with params; two parameter sets alternating through the plan cache
5. grid_vid, stats_ws, tail rows and autograd with params
6. the limits raise (Python and C ABI) and the process stays usable; no selection guard ever fired
7. the hooks with the three knobs set
"""
import ctypes
import os
import types

import pytest
import torch

import _stub_models as S
import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import PassParams, _ffi, synth
from vidcom2_amd import vidcom2 as V
from vidcom2_amd._ffi import DTYPE_CODE, check, lib, ptr

from _stage_chain import DT, FP32_TOL, case_input, digest, hook_chain, same
from conftest import load_json, make_input

pytestmark = pytest.mark.gpu

STAGE = [c for c in load_json("stage_chain_cases.json")["cases"] if c["ratio"] is not None or c["temp"] is not None]
OWN = load_json("pass_params_cases.json")["cases"]
REF_ALPHAS = [2 ** k for k in range(-3, 2)]
A4 = [0.1, 0.3, 1.0, 3.0]
KNOBS = ("VC2_CHANNEL_RATIO", "VC2_TEMP", "VC2_ALPHAS")


def dev():
    return torch.device("cuda:0")


def cid(c):
    extra = "".join(f"-{k}{c[k]:.4g}" for k in ("ratio", "temp") if c[k] is not None)
    if c.get("alphas") is not None:
        extra += f"-a{len(c['alphas'])}"
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}-{c['dtype']}-{c['dist']}-b{c['base']}{extra}"


def params_of(c):
    return PassParams(0.5 if c["ratio"] is None else c["ratio"], 0.01 if c["temp"] is None else c["temp"],
                      REF_ALPHAS if c.get("alphas") is None else c["alphas"])


def own_case(name, dtype=None, **kw):
    for c in OWN:
        if c["name"] == name and (dtype is None or c["dtype"] == dtype) and all(c[k] == v for k, v in kw.items()):
            return c
    raise KeyError((name, dtype, kw))


def own_input(c):
    x = make_input(c["F"], c["N"], c["D"], c["dtype"], c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    return x


@pytest.fixture(autouse=True)
def _default_mode(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
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


def _same_result(a, b, scores=True):
    assert a.K == b.K and torch.equal(a.ks, b.ks) and torch.equal(a.global_idx, b.global_idx)
    assert (a.rows is None) == (b.rows is None) and (a.rows is None or same(a.rows, b.rows))
    if scores:
        assert same(a.v_score, b.v_score) and same(a.f_score, b.f_score)


# ---- 1. parity with the reference ---------------------------------------------------------------------------------
def _check_against_reference(c, x, got, rows_from):
    print(cid(c), "K", got.K, "reference K", c.get("K_grid", c["K"]), "ks", got.ks.tolist(), "reference", c["ks"])
    assert got.ks.tolist() == c["ks"], "budgets"
    if c["dtype"] == "f32":
        import numpy as np
        dv = max(abs(a - b) for a, b in zip(got.v_score[0, :16].tolist(), c["v_head"]))
        df = max(abs(a - b) for a, b in zip(got.f_score[0, :16].tolist(), c["f_head"]))
        print("  fp32 score heads: max |dv|", dv, "max |df|", df, "bound", FP32_TOL)
        assert np.allclose(got.v_score[0, :16].tolist(), c["v_head"], rtol=0, atol=FP32_TOL), "v"
        assert np.allclose(got.f_score[0, :16].tolist(), c["f_head"], rtol=0, atol=FP32_TOL), "f"
    else:
        assert digest(got.v_score) == c["v_sha256"], "v"
        assert digest(got.f_score) == c["f_sha256"], "f"
    if c.get("model") == "llava_vid":
        assert got.K == c["K_grid"] and digest(got.global_idx) == c["gidx_sha256"], "grid-mapped indices"
    else:
        assert got.K == c["K"] and digest(got.global_idx) == c["keep_sha256"], "kept indices"
    assert same(got.rows, rows_from[got.global_idx.cpu()]), "rows == x[keep]"
    if "rows_sha256" in c:
        assert digest(got.rows) == c["rows_sha256"], "rows"


@pytest.mark.parametrize("c", STAGE, ids=cid)
def test_fused_pass_equals_reference_on_the_stage_chain_cases(c):
    x = case_input(c, make_input)
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    xd = x.to(dev())
    got = vc.compress(xd, c["N"], c["base"], want_scores=True, params=params_of(c))
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x), "input was modified"
    _check_against_reference(c, x, got, x)


def test_the_stage_chain_fixture_has_its_twelve_cases():
    assert len(STAGE) == 12
    assert {c["ratio"] for c in STAGE if c["ratio"] is not None} == {1 / 128, 0.25, 0.75, 1.0}
    assert {c["temp"] for c in STAGE if c["temp"] is not None} == {0.05, 0.5, 1.0}


@pytest.mark.parametrize("c", OWN, ids=cid)
def test_fused_pass_equals_reference_on_the_pass_params_cases(c):
    x = own_input(c)
    xd = x.to(dev())
    if c["model"] == "llava_vid":
        img = synth.make(c["F"], 13 * 14, c["D"], DT[c["dtype"]], c["seed"] + 5000, c["dist"])
        assert synth.sha256_tensor(img) == c["img_sha256"]
        got = vc.compress(xd, c["N"], c["base"], "grid_vid", 13, img.to(dev()), want_scores=True, params=params_of(c))
        _check_against_reference(c, x, got, img)
    else:
        got = vc.compress(xd, c["N"], c["base"], want_scores=True, params=params_of(c))
        _check_against_reference(c, x, got, x)
    assert torch.equal(xd.cpu(), x), "input was modified"


@pytest.mark.parametrize("mode", ["torch_proven", "torch_fast", "exact"])
def test_other_numerics_modes_take_params(mode):
    """torch_proven: the reference's bits as well; torch_fast / exact: the same budgets and kept tokens on these inputs
    (their scores may differ in the last bit -- no parity claim is made for them)."""
    for c in (own_case("rta", "bf16", D=3584), own_case("a8", "f16")):
        x = own_input(c)
        _ffi.set_mode(mode)
        got = vc.compress(x.to(dev()), c["N"], c["base"], want_scores=True, params=params_of(c))
        if mode == "torch_proven":
            _check_against_reference(c, x, got, x)
        else:
            assert got.rows.shape[0] == got.K == int(got.ks.sum()) and same(got.rows, x[got.global_idx.cpu()])


# ---- 2. fused pass == stage route ----------------------------------------------------------------------------------
SETTINGS = [(0.25, 0.05), (0.75, 0.5), (1.0, None), (None, 1.0), (1 / 128, 0.05)]


@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("F,N,D,dist,seed", [(8, 196, 1024, "drift", 900), (6, 144, 1536, "cancel", 901),
                                             (8, 100, 3584, "iid", 902)])
def test_fused_pass_equals_stage_route(F, N, D, dist, seed, dn, mode):
    xd = make_input(F, N, D, dn, seed, dist).to(dev())
    _ffi.set_mode(mode)
    for ratio, temp in SETTINGS:
        g = hook_chain(vc, xd, N, 0.25, ratio, temp)
        got = vc.compress(xd, N, 0.25, want_scores=True,
                          params=PassParams(0.5 if ratio is None else ratio, 0.01 if temp is None else temp))
        what = (ratio, temp)
        assert got.ks.tolist() == g["ks"], ("budgets", what)
        assert torch.equal(got.global_idx, g["keep"]), ("kept indices", what)
        assert same(got.v_score, g["v"]) and same(got.f_score, g["f"]), ("scores", what)
        assert same(got.rows, xd[g["keep"]]), ("rows", what)


# ---- 3. defaults are the default path ------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
def test_default_params_are_the_plain_pass(dn):
    F, N, D = 8, 196, 1024
    xd = make_input(F, N, D, dn, 910, "drift").to(dev())
    V.clear_plan_cache()
    a = vc.compress(xd, N, 0.25, want_scores=True)
    plans = list(V._PLAN_CACHE.values())
    assert len(plans) == 1
    b = vc.compress(xd, N, 0.25, want_scores=True, params=PassParams())
    c = vc.compress(xd, N, 0.25, want_scores=True, params=PassParams(0.5, 0.01, [2 ** k for k in range(-3, 2)]))
    _same_result(a, b)
    _same_result(a, c)
    assert list(V._PLAN_CACHE.values()) == plans and plans[0].params is None, "the plain call's cached plan is reused"
    d = vc.compress(xd, N, 0.25, want_scores=True, params=PassParams(alphas=[1.0]))
    assert len(V._PLAN_CACHE) == 2 and not same(a.v_score, d.v_score)
    ref = O.compress_indices(xd.cpu(), N, 0.25)
    assert torch.equal(a.global_idx.cpu(), ref["global_idx"])


def test_default_params_run_the_plain_kernels_at_the_target_shape():
    F, N, D = 128, 196, 3584
    xd = make_input(F, N, D, "bf16", 911, "drift").to(dev())

    def profiled(**kw):
        plan = V.CompressPlan(F, N, D, torch.bfloat16, dev(), 0.25, **kw)
        plan.enqueue(xd)
        res = plan.finish()                               # (warm: LDS opt-ins, code objects)
        _ffi.profile_enable(True)
        try:
            _ffi.profile_collect()
            plan.enqueue(xd)
            res = plan.finish()
            torch.cuda.synchronize()
            prof = _ffi.profile_collect()
        finally:
            _ffi.profile_enable(False)
        return res, {k: n for k, (_, n) in prof.items()}

    a, ka = profiled()
    b, kb = profiled(params=PassParams())
    print("kernels of a plain pass:", ka, "with default params:", kb)
    assert ka and ka == kb
    _same_result(a, b, scores=False)
    # the C ABI itself: a vc2_pass_params equal to the defaults (D / 2 channels, 0.01, the five scales) is that pass too
    plan = V.CompressPlan(F, N, D, torch.bfloat16, dev(), 0.25, params=PassParams(alphas=[1.0]))
    plan._cparams = V._CPassParams(D // 2, 0.01, 5, (ctypes.c_double * 16)(*REF_ALPHAS))
    plan.enqueue(xd)
    _same_result(a, plan.finish(), scores=False)


# ---- 4. compress_batch ---------------------------------------------------------------------------------------------
def test_compress_batch_with_params_same_shape():
    P = PassParams(0.25, 0.05, A4)
    clips = [make_input(8, 196, 1024, "bf16", 920 + i, ("drift", "cancel", "iid")[i % 3]).to(dev()) for i in range(5)]
    res = vc.compress_batch(clips, 196, 0.25, params=P)
    plain = vc.compress_batch(clips, 196, 0.25)
    assert len(res) == 5
    for x, r, q in zip(clips, res, plain):
        _same_result(r, vc.compress(x, 196, 0.25, params=P), scores=False)
        _same_result(q, vc.compress(x, 196, 0.25), scores=False)
    assert any(not torch.equal(r.ks, q.ks) for r, q in zip(res, plain)), "the parameters changed nothing"


def test_compress_batch_with_params_mixed_tokens_per_frame():
    P = PassParams(0.75, 0.5, [1, 2])
    shapes = [(6, 100, 1024, "bf16"), (8, 144, 1024, "bf16"), (4, 196, 1024, "bf16"), (6, 100, 1024, "bf16")]
    clips = [make_input(F, N, D, dn, 930 + i, "drift").to(dev()) for i, (F, N, D, dn) in enumerate(shapes)]
    res = vc.compress_batch(clips, [s[1] for s in shapes], 0.3, gather=False, params=P)
    for x, s, r in zip(clips, shapes, res):
        one = vc.compress(x, s[1], 0.3, gather=False, params=P)
        assert r.rows is None and r.K == one.K and torch.equal(r.ks, one.ks) and torch.equal(r.global_idx, one.global_idx)


def test_compress_batch_refuses_before_it_enqueues():
    clips = [torch.zeros(4 * 16, 64, dtype=torch.bfloat16, device=dev())] * 2
    with pytest.raises(ValueError):
        vc.compress_batch(clips, 16, 0.25, params=PassParams(1 / 128))


def test_two_parameter_sets_alternate_through_the_plan_cache():
    c = own_case("rt", "bf16", D=1024)                       # 12 x 196 x 1024, ratio 0.25, temp 0.05
    x = own_input(c)
    xd = x.to(dev())
    P = params_of(c)
    plain_ref = O.compress_indices(x, c["N"], c["base"])
    V.clear_plan_cache()
    for rnd in range(3):
        a = vc.compress(xd, c["N"], c["base"], want_scores=True, params=P)
        b = vc.compress(xd, c["N"], c["base"], want_scores=True)
        _check_against_reference(c, x, a, x)
        assert b.ks.tolist() == plain_ref["ks"].tolist() and torch.equal(b.global_idx.cpu(), plain_ref["global_idx"])
        assert same(b.v_score.cpu(), plain_ref["v"]) and same(b.rows.cpu(), x[plain_ref["global_idx"]])
        assert len(V._PLAN_CACHE) == 2, "one plan per parameter set"
    assert {p.params for p in V._PLAN_CACHE.values()} == {None, P}


# ---- 5. the other call options ---------------------------------------------------------------------------------------
def test_stats_workspace_with_params():
    from vidcom2_amd.fused import pool_stats
    P = PassParams(0.25, 0.05, A4)
    for dt, mode, H in ((torch.bfloat16, "average", 28), (torch.float16, "bilinear", 27), (torch.float32, "max", 28)):
        x = synth.make(8, H * H, 512, dt, 11).reshape(8, H * H, 512).to(dev())
        pooled, ws = pool_stats(x, H, H, mode)
        flat = pooled.flatten(0, 1)
        a = vc.compress(flat, 196, 0.25, want_scores=True, params=P)
        b = vc.compress(flat, 196, 0.25, want_scores=True, stats_ws=ws, params=P)
        _same_result(a, b)
        assert not torch.equal(a.ks, vc.compress(flat, 196, 0.25).ks) or dt == torch.float32


def test_grid_vid_with_params_and_stats():
    from vidcom2_amd.fused import pool_stats
    c = own_case("llava_vid")
    P = params_of(c)
    x = synth.make(6, 26 * 26, 256, torch.bfloat16, 12).reshape(6, 26 * 26, 256).to(dev())
    pooled, ws = pool_stats(x, 26, 26, "average")
    flat = pooled.flatten(0, 1)
    img = make_input(6, 13 * 14, 256, "bf16", 940, "drift").to(dev())
    a = vc.compress(flat, 169, 0.25, "grid_vid", 13, img, want_scores=True, params=P)
    b = vc.compress(flat, 169, 0.25, "grid_vid", 13, img, want_scores=True, stats_ws=ws, params=P)
    _same_result(a, b)
    lin = vc.compress(flat, 169, 0.25, gather=False, params=P)
    assert torch.equal(a.ks, lin.ks) and a.K == lin.K + 6 * 13 and same(a.rows, img[a.global_idx])


def test_tail_rows_with_params():
    c = own_case("a4", "bf16")
    x = own_input(c)
    xd = x.to(dev())
    tail = make_input(1, 2, c["D"], "bf16", 941, "iid").to(dev())
    got = vc.compress(xd, c["N"], c["base"], tail=tail, params=params_of(c))
    assert got.K == c["K"] and digest(got.global_idx) == c["keep_sha256"]
    assert got.rows.shape[0] == c["K"] + 2 and digest(got.rows[:c["K"]]) == c["rows_sha256"]
    assert torch.equal(got.rows[c["K"]:], tail)


def test_rows_carry_gradients_with_params():
    P = PassParams(0.75, 0.05, A4)
    x = make_input(6, 100, 1024, "bf16", 942, "drift").to(dev())
    xa = x.clone().requires_grad_(True)
    got = vc.compress(xa, 100, 0.25, params=P)
    assert got.rows.requires_grad
    g = make_input(1, got.K, 1024, "bf16", 943, "iid").to(dev())
    got.rows.backward(g)
    xb = x.clone().requires_grad_(True)
    xb[got.global_idx].backward(g)
    assert torch.equal(xa.grad, xb.grad)
    res = vc.compress_batch([xa, xa.detach()], 100, 0.25, params=P)
    assert res[0].rows.requires_grad and not res[1].rows.requires_grad and torch.equal(res[0].global_idx, got.global_idx)


# ---- 6. limits ----------------------------------------------------------------------------------------------------------
def _plain_pass_is_correct():
    x = make_input(8, 196, 1024, "bf16", 0, "drift")
    ref = O.compress_indices(x, 196, 0.25)
    got = vc.compress(x.to(dev()), 196, 0.25)
    assert got.ks.cpu().tolist() == ref["ks"].tolist() and torch.equal(got.global_idx.cpu(), ref["global_idx"])
    assert torch.equal(got.rows.cpu(), x[ref["global_idx"]])


def test_limits_raise_and_the_process_stays_usable():
    wide = torch.ones(4 * 16, 8192, dtype=torch.bfloat16, device=dev())
    with pytest.raises(NotImplementedError):              # 8192 scored channels
        vc.compress(wide, 16, 0.25, params=PassParams(1.0))
    _plain_pass_is_correct()
    vc.compress(wide, 16, 0.25, params=PassParams(0.5, 0.5))        # (4096 of 8192 channels: inside the limit)
    narrow = torch.ones(4 * 16, 64, dtype=torch.bfloat16, device=dev())
    with pytest.raises(ValueError):                       # int(64 / 128) == 0 channels
        vc.compress(narrow, 16, 0.25, params=PassParams(1 / 128))
    _plain_pass_is_correct()
    with pytest.raises(ValueError):
        V.CompressPlan(4, 16, 64, torch.bfloat16, dev(), 0.25, params=PassParams(1 / 128))
    with pytest.raises(NotImplementedError):
        vc.compress(narrow, 16, 0.25, params=PassParams(alphas=[1.0] * 17))
    _plain_pass_is_correct()


@pytest.mark.parametrize("channels,temp,alphas,n,rc", [
    (0, 0.01, [1.0], None, -1), (513, 0.01, [1.0], None, -1), (-3, 0.01, [1.0], None, -1),
    (256, 0.0, [1.0], None, -1), (256, -1.0, [1.0], None, -1), (256, float("nan"), [1.0], None, -1),
    (256, float("inf"), [1.0], None, -1), (256, 0.01, [1.0, 0.0], None, -1), (256, 0.01, [-1.0], None, -1),
    (256, 0.01, [float("inf")], None, -1), (256, 0.01, [], 0, -1), (256, 0.01, [1.0] * 16, 17, -3)])
def test_c_abi_refuses_bad_params_and_enqueues_nothing(channels, temp, alphas, n, rc):
    F, N, D = 4, 64, 512
    x = make_input(F, N, D, "bf16", 950, "drift").to(dev())
    plan = V.CompressPlan(F, N, D, torch.bfloat16, dev(), 0.25)
    plan.enqueue(x)
    good = plan.finish()
    keep = (good.K, good.global_idx.clone(), good.ks.clone())
    cp = V._CPassParams(channels, temp, len(alphas) if n is None else n,
                        (ctypes.c_double * 16)(*(list(alphas) + [1.0] * (16 - len(alphas)))))
    o = plan.out
    got = lib().vc2_compress_ex3(ptr(x), F, N, D, DTYPE_CODE[torch.bfloat16], 0.25, 0, 0, ptr(x), x.shape[0], ptr(plan.ws),
                                 plan.ws.numel(), ptr(o.rows), ptr(o.idx), plan.cap, ptr(o.ks), ptr(o.kout), None, None,
                                 None, 0, 0, None, ctypes.addressof(cp), _ffi.stream_ptr(dev()))
    assert got == rc, _ffi.last_error()
    torch.cuda.synchronize()
    assert o.kout.tolist() == [keep[0], 0] and torch.equal(o.idx[:keep[0]], keep[1]) and torch.equal(o.ks, keep[2])
    _plain_pass_is_correct()


def test_c_abi_channel_limit_is_unsupported():
    F, N, D = 3, 32, 8192
    x = make_input(F, N, D, "bf16", 951, "drift").to(dev())
    plan = V.CompressPlan(F, N, D, torch.bfloat16, dev(), 0.25)
    cp = V._CPassParams(4097, 0.01, 1, (ctypes.c_double * 16)(1.0))
    o = plan.out
    rc = lib().vc2_compress_ex3(ptr(x), F, N, D, DTYPE_CODE[torch.bfloat16], 0.25, 0, 0, ptr(x), x.shape[0], ptr(plan.ws),
                                plan.ws.numel(), ptr(o.rows), ptr(o.idx), plan.cap, ptr(o.ks), ptr(o.kout), None, None,
                                None, 0, 0, None, ctypes.addressof(cp), _ffi.stream_ptr(dev()))
    assert rc == -3, _ffi.last_error()
    _plain_pass_is_correct()


# ---- 7. hooks ------------------------------------------------------------------------------------------------------------
def _set_knobs(monkeypatch, c):
    if c["ratio"] is not None:
        monkeypatch.setenv("VC2_CHANNEL_RATIO", repr(c["ratio"]))
    if c["temp"] is not None:
        monkeypatch.setenv("VC2_TEMP", repr(c["temp"]))
    if c["alphas"] is not None:
        monkeypatch.setenv("VC2_ALPHAS", ",".join(repr(a) for a in c["alphas"]))


@pytest.mark.parametrize("c", [own_case("rta", "f16", D=1536), own_case("rta", "bf16", D=3584), own_case("a_ints"),
                               own_case("rt", "f16")], ids=cid)
def test_keep_index_functions_with_the_knobs_set(c, monkeypatch):
    import math
    from vidcom2_amd.models.qwen2_5_vl import _compute_keep_indices, _compute_keep_indices_many
    from vidcom2_amd.models.llava_hf import _keep_indices, _keep_indices_many
    from vidcom2_amd.models.qwen2_vl import _keep_index
    _set_knobs(monkeypatch, c)
    xd = own_input(c).to(dev())
    side = 2 * math.isqrt(c["N"])                          # merge size 2: tokens per frame = (h / 2) * (w / 2)
    assert (side // 2) ** 2 == c["N"]
    grid = torch.tensor([c["F"], side, side])
    keep = _compute_keep_indices(xd, grid, 2, c["base"])
    assert keep.numel() == c["K"] and digest(keep) == c["keep_sha256"]
    both = _compute_keep_indices_many([xd, xd], torch.stack([grid, grid]), 2, c["base"])
    assert torch.equal(both, torch.cat([keep, keep + xd.shape[0]]))
    assert digest(_keep_indices(xd, c["N"], c["base"])) == c["keep_sha256"]
    assert [digest(k) for k in _keep_indices_many([xd, xd], c["N"], c["base"])] == [c["keep_sha256"]] * 2
    monkeypatch.setenv("R_RATIO", str(c["base"]))
    assert digest(_keep_index(xd, grid[None], 2)) == c["keep_sha256"]
    for k in KNOBS:                                        # knobs unset again: the plain pass
        monkeypatch.delenv(k, raising=False)
    plain = _compute_keep_indices(xd, grid, 2, c["base"])
    assert torch.equal(plain, vc.compress(xd, c["N"], c["base"], gather=False).global_idx)
    assert not torch.equal(plain, keep) or plain.numel() != keep.numel()


HOOK_CASES = load_json("hook_cases.json")


def test_qwen25_prefill_with_the_knobs_set(monkeypatch):
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    c = next(k for k in HOOK_CASES["qwen2_5_vl"] if k["name"] == "one_video_bf16")
    P = PassParams(0.25, 1.0, A4)
    monkeypatch.setenv("VC2_CHANNEL_RATIO", "0.25")
    monkeypatch.setenv("VC2_TEMP", "1.0")
    monkeypatch.setenv("VC2_ALPHAS", "0.1,0.3,1.0,3.0")
    monkeypatch.setenv("R_RATIO", c["r"])
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    ids, feats, pos, mask = S.qwen_inputs(c)
    model, rec = S.make_qwen_vl_model("qwen2_5_vl", c["D"], S.DT[c["dt"]], "cuda", c["seed"])
    S.set_video_features(model, [f.to(dev()) for f in feats])
    model.forward = types.MethodType(hook, model)
    model(input_ids=ids.to(dev()), attention_mask=mask.to(dev()), position_ids=pos.to(dev()),
          pixel_values_videos=torch.zeros(1, 4, device=dev()), video_grid_thw=torch.tensor(c["grids"], device=dev()))
    seen = rec.calls[-1]
    (t, h, w), = c["grids"]
    kept = vc.compress(feats[0].to(dev()), (h * w) // 4, float(c["r"]), gather=False, params=P).global_idx.cpu()
    video_pos = (ids[0] == S.VIDEO_ID).nonzero()[:, 0]
    expect = torch.cat([(ids[0] != S.VIDEO_ID).nonzero()[:, 0], video_pos[kept]]).sort().values
    assert seen["position_ids"][0, 0].tolist() == expect.tolist()
    assert expect.tolist() != c["keep_token_indices"], "the knobs changed nothing"
    table = S.embed_table(c["D"], S.DT[c["dt"]], c["seed"])
    full = table[ids[0]].clone()
    full[video_pos] = feats[0]
    assert torch.equal(seen["inputs_embeds"][0].cpu(), full[expect])


def test_llava_prefill_with_the_knobs_set(monkeypatch):
    from vidcom2_amd.models.llava import cus_prepare_inputs_labels_for_multimodal as hook
    c = next(k for k in HOOK_CASES["llava"] if k["name"] == "ov_one_token_bf16")
    P = PassParams(0.75, 1.0, [1.0, 2.0])
    monkeypatch.setenv("R_RATIO", c["r"])
    ids, feats = S.llava_inputs(c)
    ids, feats = ids.to(dev()), feats.to(dev())
    m = S.StubLlava(c["D"], S.DT[c["dt"]], "cuda", c["seed"], c["merge"], c["newline"])
    plain = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)[4]
    m.prepare_inputs_labels_for_multimodal = types.MethodType(hook, m)
    default = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)[4]
    assert synth.sha256_tensor(default) == c["comp_sha"]           # knobs unset: the fixture's (today's) result
    monkeypatch.setenv("VC2_CHANNEL_RATIO", "0.75")
    monkeypatch.setenv("VC2_TEMP", "1.0")
    monkeypatch.setenv("VC2_ALPHAS", "1,2")
    comp = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)[4]
    n0, nv = c["prefix"], c["F"] * c["N"]
    video = plain[0, n0:n0 + nv]
    kept = vc.compress(video.contiguous(), c["N"], float(c["r"]), gather=False, params=P).global_idx
    expect = torch.cat([plain[0, :n0], video[kept], plain[0, n0 + nv:]])
    assert type(comp) is torch.Tensor and torch.equal(comp[0], expect)
    assert comp.shape != default.shape or not torch.equal(comp, default), "the knobs changed nothing"


def test_no_selection_guard_fired():
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)

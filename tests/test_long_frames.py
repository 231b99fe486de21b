"""Frames of 256 to 8192 tokens (the library's limit) against the reference's vectors and the CPU oracle.  Qwen2-VL,
Qwen2.5-VL and Qwen3-VL hand the pass h * w / merge^2 tokens per frame: 576 to 1296 at ordinary video resolutions.  Every
other fixture has N <= 324, but several code paths switch on N:

* the frame-mean replay: lds_column_short up to 512 rows, wave_column_solo (level-1 group by level-1 group) above; torch's
  cascade adds a second level at 256 rows and a third at 4096, the tail columns' (C % 32 != 0) four chains of N / 4 rows
  their second level at 1024;
* sweep 2's ORD form (16-bit, D in {1024, 3584, 4096}, N <= 512) against the margin / flag / replay form from N = 513;
* the selection engines: topk_smallest4_solo<4> / <8> up to 256 / 512 values, one-wave topk_smallest2 up to
  sel2_capacity(1, 4) = 1020, four waves above, cooperatively up to sel2_capacity(4, 8) = 8188;
* the plan geometry (stat_splits, S / S_q, sweep 3's splits, the rider frames).

The contract is test_wide_and_scalar_rows.py's: budgets and kept indices exact, half-precision scores bit-equal to the
oracle in the same mode, fp32 scores within 1e-6 of the oracle's `exact` mode (the kernels accumulate fp32 inputs in fp64).
The reference's own vectors are tests/golden/long_frame_cases.json (make_long_frame_golden.py)."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd._ffi import DTYPE_CODE, check, lib

from conftest import DT, load_json, make_input

pytestmark = pytest.mark.gpu
CASES = load_json("long_frame_cases.json")["cases"]


@pytest.fixture(autouse=True)
def _default_mode():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")


def dev():
    return torch.device("cuda:0")


def cid(c):
    return f"{c['name']}-{c['F']}x{c['N']}x{c['D']}-{c['dtype']}-{c['dist']}"


def nan_eq(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _set_modes(mode, dn):
    """GPU in `mode`; the oracle in `mode` for half precision ('torch' for 'torch_proven', which has the same results),
    in `exact` for fp32 (see the module docstring)."""
    _ffi.set_mode(mode)
    O.set_mode("exact" if dn == "f32" else "torch" if mode == "torch_proven" else mode)


def _check_vs_oracle(got, ref, x, dn, what=""):
    gi = got.global_idx.cpu()
    assert got.ks.cpu().tolist() == ref["ks"].tolist(), ("budgets", what)
    assert got.K == int(ref["global_idx"].numel()) and torch.equal(gi, ref["global_idx"]), ("kept indices", what)
    if dn == "f32":
        assert (got.v_score.cpu() - ref["v"]).abs().max().item() <= 1e-6, ("v_score", what)
        assert (got.f_score.cpu() - ref["f"]).abs().max().item() <= 1e-6, ("f_score", what)
    else:
        assert nan_eq(got.v_score, ref["v"]) and nan_eq(got.f_score, ref["f"]), ("scores", what)
    assert torch.equal(got.rows.cpu(), x[gi]), ("rows", what)


def _check_vs_golden(got, c, what=""):
    gi = got.global_idx.cpu()
    assert got.ks.cpu().tolist() == c["ks"], ("budgets", what)
    assert got.K == c["K"] and synth.sha256_tensor(gi) == c["idx_sha256"], ("kept indices", what)
    assert synth.sha256_tensor(got.rows) == c["out_sha256"], ("rows", what)
    if c["dtype"] == "f32":
        assert np.allclose(got.v_score[0, :16].cpu().tolist(), c["v_head"], rtol=0, atol=1e-5), ("v_score", what)
        assert np.allclose(got.f_score[0, :16].cpu().tolist(), c["f_head"], rtol=0, atol=1e-5), ("f_score", what)
    else:
        assert synth.sha256_tensor(got.v_score) == c["v_sha256"], ("v_score", what)
        assert synth.sha256_tensor(got.f_score) == c["f_sha256"], ("f_score", what)


def _input(c):
    x = make_input(c["F"], c["N"], c["D"], c["dtype"], c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"]
    return x


def _with_env(key, value, fn):
    old = os.environ.get(key)
    try:
        os.environ[key] = value
        return fn()
    finally:
        if old is None:
            del os.environ[key]
        else:
            os.environ[key] = old


# ---- a. the reference's own vectors ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["torch", "torch_proven", "exact"])
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_reference_cases(c, mode):
    """Modes 'torch' and 'torch_proven': HIP == the reference (budgets, kept indices, rows; half-precision scores bit for
    bit); fp32 also == the oracle's exact mode.  Mode 'exact': HIP == the oracle's exact mode."""
    x = _input(c)
    xd = x.to(dev())
    keep = xd.clone()
    _set_modes(mode, c["dtype"])
    got = vc.compress(xd, c["N"], c["base"], want_scores=True)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "input was modified"
    if mode != "exact":
        _check_vs_golden(got, c, mode)
    if mode == "exact" or c["dtype"] == "f32":
        _check_vs_oracle(got, O.compress_indices(x, c["N"], c["base"]), x, c["dtype"], mode)
    if mode == "torch":
        chan = vc.vidcom2.low_var_channel_order(xd)
        assert synth.sha256_tensor(chan.cpu()) == c["chan_sha256"]


# ---- b. every frame mean through the replay ---------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("D", [256, 200, 328])
@pytest.mark.parametrize("N", [513, 1021, 4097, 8192])
def test_replay_everything(N, D, dn):
    """Debug mode 2 replays torch's order for every centre mean: each frame mean of these frames goes through
    wave_column_solo (N > 512), the level-1 groups of the tail columns (D = 200: C = 100; 328: C = 164) as well."""
    F = 3 if N <= 1021 else 2
    x = make_input(F, N, D, dn, 50 + N % 7, "cancel" if dn == "f16" else "drift")
    O.set_mode("torch")
    ref = O.compress_indices(x, N, 0.25)
    assert lib().vc2_set_mode(2) == 0
    got = vc.compress(x.to(dev()), N, 0.25, want_scores=True)
    torch.cuda.synchronize()
    _check_vs_oracle(got, ref, x, dn)


# ---- c. the replay path really ran -----------------------------------------------------------------------------------
def _pass_counters(c, xd):
    """One default-mode pass on a plan of our own, then its workspace's ticket words (vc2_pass_counters)."""
    dtype = DT[c["dtype"]]
    plan = vc.vidcom2.CompressPlan(c["F"], c["N"], c["D"], dtype, dev(), c["base"], want_scores=True)
    plan.enqueue(xd)
    got = plan.finish()
    out8 = (ctypes.c_int32 * 8)()
    check(lib().vc2_pass_counters(c["F"], c["N"], c["D"], DTYPE_CODE[dtype], ctypes.c_void_p(plan.ws.data_ptr()), out8),
          "vc2_pass_counters")
    return got, list(out8)


DISCRIMINATING = [c for c in CASES if c["dtype"] == "f16" and c["dist"] == "cancel" and c["N"] > 512
                  and c["centres_exact_ne"]["frame"] > 0]


@pytest.mark.parametrize("c", DISCRIMINATING, ids=cid)
def test_frame_replays_are_listed_on_cancel_frames(c):
    """Where fp64-exact frame means differ from the reference's (centres_exact_ne), the default mode must list
    boundary-near frame means for replay in torch's order.  Ticket word 7 (kTkFrameReplays) is the length of that list:
    k_frame_centres adds its entries there, and the rider waves of the fused k_video_centre launch replay exactly those
    entries.  (Frames with a corrected norm go on a separate list, counted in word 8, which vc2_pass_counters does not
    return.)  The result equals the reference's."""
    xd = _input(c).to(dev())
    got, out8 = _pass_counters(c, xd)
    _check_vs_golden(got, c)
    print(cid(c), "pass counters", out8)
    assert out8[7] > 0, out8


def test_ord_form_lists_no_frame_replay():
    """The counter-example to the test above: at N = 512 (D = 3584, fp16) sweep 2 adds the frames in torch's own order
    (ORD form), so no frame mean is listed for replay even on `cancel` frames -- and the result is the reference's."""
    c = next(c for c in CASES if (c["N"], c["D"], c["dtype"], c["dist"]) == (512, 3584, "f16", "cancel"))
    assert lib().vc2_selftest_ord_pieces(c["F"], c["N"], c["D"], DTYPE_CODE[torch.float16], None, 0) > 0
    got, out8 = _pass_counters(c, _input(c).to(dev()))
    _check_vs_golden(got, c)
    assert out8[7] == 0, out8


# ---- d. both forms of sweep 2 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ord_form", ["1", "0"])
@pytest.mark.parametrize("shape", [(3, 257, "f16", "cancel"), (3, 257, "bf16", "drift"), (3, 512, "f16", "cancel"),
                                   (3, 512, "bf16", "drift")], ids=lambda s_: "x".join(map(str, s_)))
def test_both_sweep2_forms(shape, ord_form):
    """VC2_S2_ORD = 1 (ord_frame_sum_clean<33> from 256 rows) and 0 (margins and replays through lds_column_short) at
    D = 3584: the oracle's result, and at N = 512 the reference's."""
    F, N, dn, dist = shape
    D = 3584
    golden = [c for c in CASES if (c["F"], c["N"], c["D"], c["dtype"], c["dist"]) == (F, N, D, dn, dist)]
    x = _input(golden[0]) if golden else make_input(F, N, D, dn, 60, dist)
    O.set_mode("torch")
    ref = O.compress_indices(x, N, 0.25)
    got = _with_env("VC2_S2_ORD", ord_form, lambda: vc.compress(x.to(dev()), N, 0.25, want_scores=True))
    torch.cuda.synchronize()
    _check_vs_oracle(got, ref, x, dn, f"VC2_S2_ORD={ord_form}")
    if golden:
        _check_vs_golden(got, golden[0], f"VC2_S2_ORD={ord_form}")


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_ord_form_ends_at_512_tokens(dn):
    L = lib()
    for D in (1024, 3584, 4096):
        assert L.vc2_selftest_ord_pieces(3, 512, D, DTYPE_CODE[DT[dn]], None, 0) > 0
        assert L.vc2_selftest_ord_pieces(3, 513, D, DTYPE_CODE[DT[dn]], None, 0) == 0


# ---- e. selection edges in the full pass -------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
@pytest.mark.parametrize("N", [256, 257, 512, 513, 1020, 1021, 8188, 8189, 8192])
def test_selection_edges(N, dn):
    """Each selection engine at its edges: constant input (every score ties: the kept set is decided by the tie order
    alone) and base 1.0 (budgets of N).  No loop bound of the selection replay may expire.
    In bf16 a scale of 1.0 times N = 8188 or 8189 rounds to 8192: the reference's torch.topk raises "selected index k
    out of range" there, and so must the pass (one clip or a batch) -- not return min(k, N) tokens."""
    _set_modes("torch", dn)
    D = 64
    xs = [torch.full((2 * N, D), 0.5, dtype=DT[dn]), make_input(2, N, D, dn, 70, "drift")]
    raised = 0
    for x in xs:
        for base in (0.25, 1.0):
            try:
                ref = O.compress_indices(x, N, base)
            except RuntimeError as e:
                assert "k out of range" in str(e) and dn == "bf16" and base == 1.0 and N in (8188, 8189)
                raised += 1
                for call in (lambda: vc.compress(x.to(dev()), N, base), lambda: vc.compress_batch([x.to(dev())] * 2, N, base)):
                    with pytest.raises(RuntimeError, match="selected index k out of range"):
                        call()
                continue
            got = vc.compress(x.to(dev()), N, base, want_scores=True)
            torch.cuda.synchronize()
            _check_vs_oracle(got, ref, x, dn, base)
    assert raised == (2 if dn == "bf16" and N in (8188, 8189) else 0)
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)


# ---- f. the frame-sharded pass -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [2, 3])
def test_frame_sharded_long_frames(P):
    """6 x 1296 x 3584 fp16 `cancel` split over P logical ranks (test_sharded's emulation on one GPU): the scores are the
    unsharded pass's bits, and budgets, kept indices and rows the reference's."""
    from test_sharded import _emulate_ranks_on_one_gpu
    c = next(c for c in CASES if c["name"] == "sharded1296")
    x = _input(c)
    xd = x.to(dev())
    whole = vc.compress(xd, c["N"], c["base"], want_scores=True)
    _check_vs_golden(whole, c, "unsharded")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res, st = _emulate_ranks_on_one_gpu(xd, c["F"], c["N"], c["D"], torch.float16, c["base"], P, dev())
    assert all(s.vc_fragile == 0 for s in st)
    assert torch.equal(torch.cat([s.total for s in st]), (whole.v_score + whole.f_score).float().flatten())
    ks = torch.cat([r.ks for r in res]).cpu()
    gidx = torch.cat([r.global_idx for r in res]).cpu()
    assert ks.tolist() == c["ks"] and synth.sha256_tensor(gidx) == c["idx_sha256"]
    assert torch.equal(torch.cat([r.rows for r in res]), whole.rows)


# ---- g. the limit ------------------------------------------------------------------------------------------------------
def test_frames_over_the_limit_are_refused():
    """N = 8193 is refused with the library's own error before anything is launched; the next valid call is right."""
    c = next(c for c in CASES if (c["N"], c["D"], c["dtype"]) == (8192, 256, "bf16"))
    x = _input(c)
    xd = x.to(dev())

    def valid():
        _check_vs_golden(vc.compress(xd, c["N"], c["base"], want_scores=True), c, "after")

    valid()
    for dn in ("bf16", "f16", "f32"):
        bad = torch.zeros(2 * 8193, 256, dtype=DT[dn], device=dev())
        with pytest.raises(NotImplementedError, match="8193 > 8192 tokens per frame"):
            vc.compress(bad, 8193, 0.25)
        valid()


# ---- h. a real frame through the hook --------------------------------------------------------------------------------
def test_qwen25_hook_at_a_real_frame_grid(monkeypatch):
    """The Qwen2.5-VL hook on a stub model of a 7B model's width, at a video grid of [4, 48, 48] (576 tokens per frame):
    the device pass gives the prompt the hook's CPU definition (the oracle under the same hook) gives."""
    from test_hooks import _run_qwen, _use_oracle
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", "0.25")
    c = dict(name="frame576", D=3584, dt="bf16", seed=41, r="0.25", grids=[[4, 48, 48]], prefix=11, between=0,
             suffix=7, mask="2d")
    _, got, _ = _run_qwen("qwen2_5_vl", hook, c, "cuda")
    _use_oracle(monkeypatch)
    _, want, _ = _run_qwen("qwen2_5_vl", hook, c, "cpu")
    assert torch.equal(got["position_ids"].cpu(), want["position_ids"])
    assert got["position_ids"].shape[-1] < 11 + 7 + 4 * 576                       # something was pruned
    assert torch.equal(got["inputs_embeds"].cpu(), want["inputs_embeds"])
    assert torch.equal(got["attention_mask"].cpu(), want["attention_mask"])

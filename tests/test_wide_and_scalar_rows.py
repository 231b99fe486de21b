"""The two kinds of row the library admits that the fixture suites did not reach, against the CPU oracle:

* 16-bit D in (4096, 8192] -- the hidden sizes of Qwen2.5-VL-32B / Qwen3-VL-32B (5120) and Qwen2.5-VL-72B /
  LLaVA-Video-72B (8192).  Above 4096 the pass takes other code: the LDS-round k_chan_select instead of
  k_chan_select4, no fused k_var_select, no sweep-2 ORDER rider (k > 4096), row kernels of up to 1024 threads, no
  streamlined sweep 2 at NCH 10 / 12.
* rows that are not a whole number of vectors (D % 8 != 0 in 16-bit, D % 4 != 0 in fp32): VEC = 1, the scalar
  channel loops of every sweep and replay kernel.
* the size limits (at most 1024 column vectors per row): refused with the library's own error, the last legal
  shapes accepted.

The contract is test_full_pass's: budgets, kept indices and (half precision) scores bit-equal to the oracle in the
same mode; fp32 scores within 1e-6 and fp32 kept indices against the oracle's `exact` mode (the kernels accumulate
fp32 inputs in fp64 in either mode, DESIGN.md "Numerics contract")."""
import os

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth

from conftest import DT, case_id, load_json, make_input

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


# ---- the reference's own vectors at these shapes (tests/golden/wide_scalar_cases.json) ------------------------------
@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("c", load_json("wide_scalar_cases.json")["cases"], ids=case_id)
def test_reference_cases(c, mode):
    """As test_full_pass: HIP == the oracle in the same mode, and == the reference's kept indices, rows and
    (half precision) score digests."""
    _set_modes(mode, c["dtype"])
    x = make_input(c["F"], c["N"], c["D"], c["dtype"], c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"]
    got = vc.compress(x.to(dev()), c["N"], c["base"], want_scores=True)
    chan = vc.vidcom2.low_var_channel_order(x.to(dev()))
    torch.cuda.synchronize()
    _check_vs_oracle(got, O.compress_indices(x, c["N"], c["base"]), x, c["dtype"])
    assert synth.sha256_tensor(chan.cpu()) == c["chan_sha256"]
    assert got.ks.cpu().tolist() == c["ks"]
    if mode == "torch" or c["stable"]:
        assert got.global_idx.cpu().tolist() == c["global_idx"]
        assert synth.sha256_tensor(got.rows) == c["out_sha256"]
    if mode == "torch" and c["dtype"] != "f32":
        assert synth.sha256_tensor(got.v_score) == c["v_sha256"] and synth.sha256_tensor(got.f_score) == c["f_sha256"]


# ---- 16-bit D in (4096, 8192]: the full pass --------------------------------------------------------------------
WIDE_D = [4104, 5120, 6144, 8184, 8192]          # 4104: just past the seam, not a multiple of 512; 8184: CV = 1023
WIDE_SHAPES = [(6, 196, "drift", 0.25), (9, 100, "iid", 0.125), (5, 324, "cancel", 0.25)]
WIDE_CASES = [(D, dn, *WIDE_SHAPES[(i + j) % len(WIDE_SHAPES)])
              for i, D in enumerate(WIDE_D) for j, dn in enumerate(("bf16", "f16"))]


@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wide_rows_full_pass(case, mode):
    D, dn, F, N, dist, base = case
    _set_modes(mode, dn)
    x = make_input(F, N, D, dn, 3, dist)
    ref = O.compress_indices(x, N, base)
    xd = x.to(dev())
    keep = xd.clone()
    got = vc.compress(xd, N, base, want_scores=True)
    chan = vc.vidcom2.low_var_channel_order(xd)
    torch.cuda.synchronize()
    assert torch.equal(xd, keep), "input was modified"
    _check_vs_oracle(got, ref, x, dn)
    assert torch.equal(chan.cpu(), ref["chan_idx"]), "channel order differs from the oracle's"


def _launch_forms(xd, N):
    keys = ("VC2_SEL4", "VC2_VARSEL")
    old = {k: os.environ.get(k) for k in keys}
    outs = []
    try:
        for form in ({}, {"VC2_VARSEL": "0"}, {"VC2_SEL4": "0"}):
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(form)
            r = vc.compress(xd, N, 0.25, want_scores=True)
            chan = vc.vidcom2.low_var_channel_order(xd)
            torch.cuda.synchronize()
            outs.append((form, r, chan))
    finally:
        for k in keys:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]
    return outs


@pytest.mark.parametrize("shape", [(7, 64, 5120, "bf16", "drift"), (5, 100, 5120, "f16", "cancel"),
                                   (4, 196, 8192, "bf16", "iid"), (6, 49, 8192, "f16", "drift"),
                                   (8, 100, 4096, "f32", "drift"), (5, 64, 4092, "f32", "iid")],
                         ids=lambda s_: "x".join(map(str, s_)))
def test_wide_launch_forms_agree(shape):
    """The VC2_SEL4 / VC2_VARSEL switches force the routes every D > 4096 (and every fp32) pass takes anyway: all three
    forms give the same channel order, scores, budgets and kept indices, and the oracle's.  fp32 at its own edge:
    D = 4096 (CV = 1024) and 4092 (CV = 1023, TPB = 1024 with one idle lane)."""
    F, N, D, dn, dist = shape
    _set_modes("torch", dn)
    x = make_input(F, N, D, dn, 17, dist)
    ref = O.compress_indices(x, N, 0.25)
    outs = _launch_forms(x.to(dev()), N)
    for form, r, chan in outs:
        _check_vs_oracle(r, ref, x, dn, form)
        assert torch.equal(chan.cpu(), ref["chan_idx"]), form


def test_wide_north_star_size():
    """A 64 x 196 x 8192 bf16 clip (a 72B model's hidden size) through test_full_size_properties' size-independent
    checks, and against the oracle."""
    F, N, D, base = 64, 196, 8192, 0.25
    x = make_input(F, N, D, "bf16", 0, "drift")
    xd = x.to(dev())
    a = vc.compress(xd, N, base, want_scores=True)
    b = vc.compress(xd, N, base)
    assert torch.equal(a.global_idx, b.global_idx) and torch.equal(a.ks, b.ks)          # deterministic
    ks, gi = a.ks.cpu(), a.global_idx.cpu()
    assert a.K == int(ks.sum()) and (ks >= 1).all() and (ks <= N).all()
    assert abs(a.K - base * F * N) <= 0.02 * base * F * N + F                             # budget conserved
    assert bool((gi[1:] > gi[:-1]).all())                                                  # globally ascending
    assert torch.equal(torch.bincount(gi // N, minlength=F), ks)                           # k_f per frame
    assert torch.equal(a.rows, xd[a.global_idx])                                           # gather = index
    c = vc.compress(xd * 2, N, base)                                                       # power-of-two scaling
    assert torch.equal(c.global_idx, a.global_idx) and torch.equal(c.ks, a.ks)
    O.set_mode("torch")
    _check_vs_oracle(a, O.compress_indices(x, N, base), x, "bf16")


# ---- VEC = 1: rows that are not a whole number of vectors ---------------------------------------------------------
SCALAR_SHAPES = [(5, 33), (4, 49), (3, 169)]
SCALAR_DISTS = ("drift", "iid", "cancel")
SCALAR_CASES = [(D, dn, *SCALAR_SHAPES[(i + j) % 3], SCALAR_DISTS[(i + 2 * j) % 3])
                for j, dn in enumerate(("bf16", "f16", "f32"))
                for i, D in enumerate([7, 100, 1001, 1020] + ([1022] if dn == "f32" else []))]


@pytest.mark.parametrize("mode", ["torch", "exact"])
@pytest.mark.parametrize("case", SCALAR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_scalar_rows_full_pass(case, mode):
    D, dn, F, N, dist = case
    _set_modes(mode, dn)
    x = make_input(F, N, D, dn, 8, dist)
    ref = O.compress_indices(x, N, 0.25)
    xd = x.to(dev())
    got = vc.compress(xd, N, 0.25, want_scores=True)
    chan = vc.vidcom2.low_var_channel_order(xd)
    torch.cuda.synchronize()
    _check_vs_oracle(got, ref, x, dn)
    assert torch.equal(chan.cpu(), ref["chan_idx"])


def test_scalar_rows_degenerate_inputs():
    """test_degenerate_inputs at a VEC = 1 width (D = 100): constant input (pure tie-breaking) and all-zero rows
    (fp16 NaN scores)."""
    D = 100
    for dn in ("f32", "bf16"):
        x = torch.full((4 * 49, D), 0.5, dtype=DT[dn])
        got = vc.compress(x.to(dev()), 49, 0.25)
        ref = O.compress_indices(x, 49, 0.25)
        assert got.ks.cpu().tolist() == ref["ks"].tolist() and torch.equal(got.global_idx.cpu(), ref["global_idx"])
    for dn in ("f16", "bf16"):
        x = synth.make(3, 49, D, DT[dn], 0, "iid")
        x[5] = 0
        x[60] = 0
        got = vc.compress(x.to(dev()), 49, 0.25, want_scores=True)
        ref = O.compress_indices(x, 49, 0.25)
        assert nan_eq(got.v_score, ref["v"]) and nan_eq(got.f_score, ref["f"])
        assert got.ks.cpu().tolist() == ref["ks"].tolist() and torch.equal(got.global_idx.cpu(), ref["global_idx"])


# ---- the size limits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dn", [(8200, "bf16"), (8200, "f16"), (1030, "bf16"), (4100, "f32"), (1026, "f32"),
                                  (8193, "bf16"), (8193, "f32"), (16384, "bf16")])
def test_rows_over_the_limit_are_refused(D, dn):
    """More than 1024 column vectors per row (8 elements per vector in 16-bit, 4 in fp32, 1 when D is not a multiple):
    NotImplementedError with the plan's message, before anything is launched."""
    x = torch.zeros(2 * 16, D, dtype=DT[dn], device=dev())
    with pytest.raises(NotImplementedError, match=r"column vectors per row; at most 1024 are supported"):
        vc.compress(x, 16, 0.25)


@pytest.mark.parametrize("D,dn", [(8192, "bf16"), (8192, "f16"), (4096, "f32"), (1020, "bf16"), (1023, "f16"),
                                  (1023, "f32")])
def test_rows_at_the_limit_run(D, dn):
    x = synth.make(2, 16, D, DT[dn], 1, "iid").to(dev())
    r = vc.compress(x, 16, 0.25)
    assert r.K == int(r.ks.sum()) and torch.equal(r.rows, x[r.global_idx])


# ---- what runs downstream of the pass at wide D -------------------------------------------------------------------
def test_wide_compress_batch_matches_sequential():
    shapes = [(6, 196, 5120), (4, 196, 5120), (6, 196, 5120)]
    xs = [make_input(F, N, D, "bf16", 40 + i, "drift").cuda() for i, (F, N, D) in enumerate(shapes)]
    want = [vc.vidcom2.compress(x, 196, 0.25) for x in xs]
    for lanes in (1, 3):
        got = vc.compress_batch(xs, 196, 0.25, in_flight=lanes)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.K == w.K and torch.equal(g.global_idx, w.global_idx) and torch.equal(g.ks, w.ks)
            assert torch.equal(g.rows, w.rows)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("D", [5120, 8192])
def test_wide_gather_scatter_and_repad_match_indexing(D, dt):
    from vidcom2_amd.fused import gather_scatter, repad_rows
    from vidcom2_amd.models._prefill_prune import _gather_slots
    g = torch.Generator().manual_seed(D)
    srcs = [torch.randn(120, D, generator=g).to(dt).cuda() for _ in range(2)]
    idx = torch.randint(0, 120, (77,), generator=g).cuda()
    tail = torch.randn(1, D, generator=g).to(dt).cuda()
    out = gather_scatter(srcs, idx, tail=tail)
    assert torch.equal(out[0], torch.cat((srcs[0][idx], tail))) and torch.equal(out[1], srcs[1][idx])
    B, S, Sp = 2, 90, 70
    src = torch.randn(B, S, D, generator=g).to(dt)
    keep = torch.randint(0, S, (B, Sp), generator=g)
    keep[0, :5] = -1
    keep[1, 60:] = -1
    assert torch.equal(repad_rows(src.cuda(), keep.cuda(), check=True).cpu(), _gather_slots(src, keep, 0))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("mode", ["average", "max", "bilinear"])
@pytest.mark.parametrize("D", [5120, 8192])
def test_wide_pool_stats_bits_match_torch_pooling(D, mode, dt):
    """get_2dPool fused with sweep 1 at wide D: the pooled rows are torch's bits, and the pass on the pooled tensor
    with the fused statistics equals the pass without them.  fp32 rows this wide are over the limit: refused."""
    from test_fused import _torch_pool
    from vidcom2_amd.fused import pool_stats
    H = 14
    g = torch.Generator().manual_seed(D + H)
    x = torch.randn(3, H * H, D, generator=g).to(dt)
    if dt == torch.float32:
        with pytest.raises(NotImplementedError, match=r"column vectors per row; at most 1024 are supported"):
            pool_stats(x.cuda(), H, H, mode)
        return
    out, ws = pool_stats(x.cuda(), H, H, mode)
    want = _torch_pool(x, H, H, mode)
    it = torch.int32 if dt == torch.float32 else torch.int16
    assert out.shape == want.shape and torch.equal(out.cpu().view(it), want.view(it))
    flat = out.flatten(0, 1)
    n = out.shape[1]
    a = vc.compress(flat, n, 0.25, want_scores=True)
    b = vc.compress(flat, n, 0.25, want_scores=True, stats_ws=ws)
    assert a.K == b.K and torch.equal(a.global_idx, b.global_idx) and torch.equal(a.ks, b.ks)
    assert torch.equal(a.rows, b.rows) and nan_eq(a.v_score, b.v_score) and nan_eq(a.f_score, b.f_score)


def test_wide_qwen25_hook_matches_its_cpu_definition(monkeypatch):
    """The Qwen2.5-VL hook on a stub model with a 32B model's hidden size: the device pass gives the prompt the
    hook's CPU definition (the oracle under the same hook) gives, for a batch of one."""
    from test_hooks import _run_qwen, _use_oracle
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", "0.25")
    c = dict(name="wide5120", D=5120, dt="bf16", seed=31, r="0.25", grids=[[6, 12, 12]], prefix=11, between=0,
             suffix=7, mask="2d")
    _, got, _ = _run_qwen("qwen2_5_vl", hook, c, "cuda")
    _use_oracle(monkeypatch)
    _, want, _ = _run_qwen("qwen2_5_vl", hook, c, "cpu")
    assert torch.equal(got["position_ids"].cpu(), want["position_ids"])
    assert got["position_ids"].shape[-1] < 11 + 7 + 6 * 36                        # something was pruned
    assert torch.equal(got["inputs_embeds"].cpu(), want["inputs_embeds"])
    assert torch.equal(got["attention_mask"].cpu(), want["attention_mask"])

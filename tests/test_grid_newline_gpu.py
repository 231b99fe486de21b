"""GPU: LLaVA-Video's kept rows gathered without the newline stream (`newline=` of compress / CompressPlan.enqueue /
map_features, k_gather_rows_grid; the hook's route).

The expected value is built on the CPU from the definition of the stream add_token_per_grid builds,

    img = cat((flat.view(F, h, h, D), nl.expand(F, h, 1, D)), 2).reshape(F*h*(h+1), D)

and the new route must equal BOTH today's route, compress(x, ..., img_feat=img), in budgets, K, mapped indices, scores and
rows, AND img[global_idx] with the indices of the CPU oracle (test_grid_mapping._grid_ref).  Rows are compared as integer
bit patterns: the newline vector carries -0.0, inf, a NaN with a payload and a subnormal."""
import os
import types

import pytest
import torch

import _stub_models as S
import oracle as O
import vidcom2_amd as vc
from conftest import DT, load_json, make_input
from test_grid_mapping import _grid_ref
from vidcom2_amd import _ffi, synth
from vidcom2_amd.vidcom2 import MODEL_SPECS, CompressPlan, PassParams, _prep_newline

pytestmark = pytest.mark.gpu

IT = {"f32": torch.int32, "bf16": torch.int16, "f16": torch.int16}
# (-0.0, +inf, a NaN with a payload, the smallest subnormal) as bit patterns of each dtype
SPECIAL = {"f32": [-0x80000000, 0x7F800000, 0x7FA00123, 0x00000001], "bf16": [-0x8000, 0x7F80, 0x7FA5, 0x0001],
           "f16": [-0x8000, 0x7C00, 0x7D23, 0x0001]}


@pytest.fixture(autouse=True)
def _modes():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("torch")


def dev():
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(bits(a), bits(b)), what


def newline_vec(D, dn, seed):
    """[D] newline vector: random values with the four special bit patterns in its first elements."""
    nl = torch.randn(D, generator=torch.Generator().manual_seed(seed)).to(DT[dn])
    b = nl.view(IT[dn])
    b[:4] = torch.tensor(SPECIAL[dn], dtype=torch.int64).to(IT[dn])
    return nl


def img_of(flat, nl, F, h):
    D = flat.shape[1]
    return torch.cat((flat.view(F, h, h, D), nl.reshape(D).expand(F, h, 1, D)), 2).reshape(F * h * (h + 1), D)


def reference(x, nl, h, base, dn):
    """(img, the oracle's pass over x with img): built once per input, on the CPU."""
    F = x.shape[0] // (h * h)
    O.set_mode("torch" if dn != "f32" else "exact")
    img = img_of(x, nl, F, h)
    # (_grid_ref checks itself against the oracle's vidcom2_compression with torch.equal, which a NaN fails: that check gets
    #  the stream of a NaN-free newline; the indices do not depend on the stream)
    return img, _grid_ref(x, h, base, img_of(x, torch.nan_to_num(nl.float()).to(nl.dtype), F, h))


def whole_stream(res, img):
    """Every token kept: the K rows are the whole stream, each frame's newline rows behind its tokens -- a permutation
    of the stream's rows that global_idx names."""
    gi = res.global_idx.cpu()
    order = torch.argsort(gi)
    assert torch.equal(gi[order], torch.arange(img.shape[0]))
    same_bits(res.rows.cpu()[order], img, "the whole stream")


def same_pass(new, old, what=""):
    """The new route against today's: budgets, K, mapped indices, scores and rows."""
    assert new.K == old.K and torch.equal(new.ks, old.ks), ("budgets / K", what)
    assert torch.equal(new.global_idx, old.global_idx), ("mapped indices", what)
    for a, b in ((new.v_score, old.v_score), (new.f_score, old.f_score)):
        assert (a is None) == (b is None)
        if a is not None:
            same_bits(a, b, ("scores", what))
    assert (new.rows is None) == (old.rows is None)
    if new.rows is not None:
        same_bits(new.rows, old.rows, ("rows", what))


def check(x, nl, h, base, dn, nl_dev=None, **kw):
    """HIP with newline= against HIP with img_feat= and against img[oracle indices]; the inputs come back unmodified."""
    F = x.shape[0] // (h * h)
    img, ref = reference(x, nl, h, base, dn)
    xd, imgd = x.to(dev()), img.to(dev())
    nld = nl.to(dev()) if nl_dev is None else nl_dev
    nl_before = nld.clone()
    old = vc.compress(xd, h * h, base, "grid_vid", h, imgd, want_scores=True, **kw)
    new = vc.compress(xd, h * h, base, "grid_vid", h, newline=nld, want_scores=True, **kw)
    torch.cuda.synchronize()
    same_bits(xd, x, "flattened_feat was modified")
    same_bits(nld, nl_before, "newline was modified")
    same_pass(new, old, (F, h, x.shape[1], dn, base))
    assert new.ks.cpu().tolist() == ref["ks"].tolist()
    assert new.K == int(ref["ks"].sum()) + F * h                       # K counts the newline rows
    assert torch.equal(new.global_idx.cpu(), ref["grid_idx"])
    assert new.rows.shape == (new.K, x.shape[1])
    same_bits(new.rows, img[ref["grid_idx"]], ("rows == img[oracle indices]", F, h, x.shape[1], dn, base))
    return new, ref, img


# ---- the smallest shapes that reach each path ----------------------------------------------------------------------
# D = 8: whole 16-byte vectors per row; D = 6: 12-byte (16-bit) / 24-byte (fp32) rows, the scalar copy.  Every h with every
# F over the (D, dtype) combinations; the three budgets (k = 1; the usual quarter; every token kept) on every shape.
SMALL = [(h, (1, 3, 5)[(i + j + k) % 3], D, dn) for i, h in enumerate((2, 3, 13)) for j, D in enumerate((8, 6))
         for k, dn in enumerate(("f32", "bf16", "f16"))]


@pytest.mark.parametrize("h,F,D,dn", SMALL, ids=lambda v: str(v))
def test_small_shapes(h, F, D, dn):
    x = make_input(F, h * h, D, dn, 100 + h + F, "drift")
    nl = newline_vec(D, dn, 7 * h + F)
    for base in (0.005, 0.25, 1.0):
        new, ref, img = check(x, nl, h, base, dn)
        if base == 0.005:                                                # k = 1 (vidcom2.py:72 clamps at 1)
            assert int(ref["ks"].min()) == 1 and (h < 13 or F > 1 or ref["ks"].tolist() == [1])
        if base == 1.0:                                                  # whole frames are kept; one frame alone has scale 1
            assert int(ref["ks"].max()) == h * h
            if F == 1:                                                   # every token kept: rows is the whole stream
                assert ref["ks"].tolist() == [h * h]                     # (every h has an F = 1 case; F > 1 with every frame
                whole_stream(new, img)                                   #  whole: test_whole_stream)


def test_every_frame_count_with_every_grid():
    assert {(h, F) for h, F, _, _ in SMALL} == {(h, F) for h in (2, 3, 13) for F in (1, 3, 5)}
    assert {(D, dn) for _, _, D, dn in SMALL} == {(D, dn) for D in (8, 6) for dn in ("f32", "bf16", "f16")}


@pytest.mark.parametrize("F,D,dn", [(16, 3584, "bf16"), (9, 5120, "f16")], ids=lambda v: str(v))
def test_model_shapes(F, D, dn):
    """LLaVA-Video-7B's row (more than one workgroup pass per row) and the D > 4096 row path."""
    x = make_input(F, 169, D, dn, 5, "drift")
    check(x, newline_vec(D, dn, 3), 13, 0.25, dn)


@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_whole_stream(dn):
    """Every score ties and base_scale = 1: every frame keeps all of its tokens (test_grid_mapping.test_constant_input),
    so `rows` is the whole stream, newline column included.  The rows differ in the channels the pass does not score
    (the half with the larger variance); the scored half is constant."""
    F, h, D = 3, 13, 8
    x = torch.full((F * h * h, D), 0.5, dtype=DT[dn])
    x[:, D // 2:] = torch.randn(F * h * h, D // 2, generator=torch.Generator().manual_seed(20)).to(DT[dn])
    new, ref, img = check(x, newline_vec(D, dn, 21), h, 1.0, dn)
    assert ref["ks"].tolist() == [h * h] * F
    whole_stream(new, img)


# ---- newline layouts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn,D", [("bf16", 8), ("f32", 8), ("f16", 64)])
def test_misaligned_and_strided_newline(dn, D):
    """A view at an odd element offset: its pointer is not 16-byte aligned and it is NOT cloned -- the rows it fills take
    the scalar copy.  A non-contiguous view (every other element) is copied.  Both give the bits of the aligned vector."""
    F, h = 3, 3
    x = make_input(F, h * h, D, dn, 41, "drift")
    nl = newline_vec(D, dn, 42)
    buf = torch.zeros(D + 1, dtype=DT[dn], device=dev())
    buf[1:] = nl.to(dev())
    odd = buf[1:]
    assert odd.data_ptr() % 16 != 0 and odd.is_contiguous()
    assert _prep_newline(odd, D, DT[dn], dev()).data_ptr() == odd.data_ptr()          # handed on as it is
    check(x, nl, h, 0.25, dn, nl_dev=odd)
    wide = torch.zeros(2 * D, dtype=DT[dn], device=dev())
    wide[::2] = nl.to(dev())
    strided = wide[::2]
    assert not strided.is_contiguous()
    check(x, nl, h, 0.25, dn, nl_dev=strided)
    check(x, nl, h, 0.25, dn, nl_dev=nl.to(dev())[None])                              # [1, D]


# ---- behaviour -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["bf16", "f32"])
def test_two_newlines_through_one_cached_plan(dn):
    """The pointer belongs to the call: two one-shot passes on one cached plan, and two enqueues of one CompressPlan,
    with different vectors each write their own -- and the first result stays what it was."""
    F, h, D = 3, 13, 64
    x = make_input(F, h * h, D, dn, 61, "drift")
    na, nb = newline_vec(D, dn, 1), -newline_vec(D, dn, 2) - 3
    ia, ra = reference(x, na, h, 0.25, dn)
    ib, rb = reference(x, nb, h, 0.25, dn)
    xd = x.to(dev())
    a = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=na.to(dev()))
    b = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=nb.to(dev()))
    same_bits(a.rows, ia[ra["grid_idx"]], "first call, after the second")
    same_bits(b.rows, ib[rb["grid_idx"]], "second call")
    plan = CompressPlan(F, h * h, D, DT[dn], dev(), 0.25, "grid_vid", h)
    for nl, img, ref in ((na, ia, ra), (nb, ib, rb), (na, ia, ra)):
        plan.rows.fill_(float("nan"))
        plan.enqueue(xd, newline=nl.to(dev()))
        got = plan.finish()
        assert torch.equal(got.global_idx.cpu(), ref["grid_idx"])
        same_bits(got.rows, img[ref["grid_idx"]], "re-used plan")
    assert not any(torch.is_tensor(v) and v.numel() == D and v.dtype == DT[dn] for v in vars(plan).values())


@pytest.mark.parametrize("dn", ["bf16", "f16", "f32"])
def test_fused_pool_statistics(dn):
    """fused.pool_stats, then compress(..., stats_ws=, newline=): the pass starts behind sweep 1."""
    from vidcom2_amd.fused import pool_stats
    F, D, h, H = 4, 64, 13, 26
    g = torch.Generator().manual_seed(9)
    feat = torch.randn(F, H * H, D, generator=g).to(DT[dn]).to(dev())
    nl = newline_vec(D, dn, 10)
    out1, ws1 = pool_stats(feat, H, H, "average")
    out2, ws2 = pool_stats(feat, H, H, "average")
    f1, f2 = out1.reshape(-1, D), out2.reshape(-1, D)
    assert ws2._vc2_stats_for == (F, h * h, D, DT[dn], f2.data_ptr())
    pooled = out1.cpu().reshape(-1, D)
    img, ref = reference(pooled, nl, h, 0.25, dn)
    old = vc.compress(f1, h * h, 0.25, "grid_vid", h, img.to(dev()), want_scores=True, stats_ws=ws1)
    new = vc.compress(f2, h * h, 0.25, "grid_vid", h, newline=nl.to(dev()), want_scores=True, stats_ws=ws2)
    same_pass(new, old, "stats_ws")
    assert torch.equal(new.global_idx.cpu(), ref["grid_idx"])
    same_bits(new.rows, img[ref["grid_idx"]], "stats_ws rows")


def test_score_dtype_and_params_against_todays_route():
    F, h, D = 5, 13, 128
    x = make_input(F, h * h, D, "bf16", 71, "drift")
    nl = newline_vec(D, "bf16", 72)
    xd, nld, imgd = x.to(dev()), nl.to(dev()), img_of(x, nl, F, h).to(dev())
    for kw in (dict(score_dtype=torch.float32), dict(params=PassParams(0.25, 0.05, (0.5, 1.0, 4.0))),
               dict(score_dtype=torch.float32, params=PassParams(channel_ratio=0.75))):
        old = vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, want_scores=True, **kw)
        new = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=nld, want_scores=True, **kw)
        same_pass(new, old, kw)
        same_bits(new.rows, imgd[new.global_idx], kw)


def test_gather_false_and_tail():
    F, h, D, dn = 3, 3, 8, "bf16"
    x = make_input(F, h * h, D, dn, 81, "drift")
    nl = newline_vec(D, dn, 82)
    img, ref = reference(x, nl, h, 0.25, dn)
    xd, nld = x.to(dev()), nl.to(dev())
    a = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=nld, gather=False)          # accepted and unused
    assert a.rows is None and torch.equal(a.global_idx.cpu(), ref["grid_idx"]) and a.ks.cpu().tolist() == ref["ks"].tolist()
    tail = newline_vec(D, dn, 83).to(dev())[None]
    b = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=nld, tail=tail)               # tail rows behind the kept ones
    same_bits(b.rows, torch.cat((img[ref["grid_idx"]], tail.cpu())), "rows + tail")


@pytest.mark.parametrize("h,D,dn", [(3, 8, "f32"), (13, 6, "f16"), (13, 64, "bf16")])
def test_map_features(h, D, dn):
    """The stage API: map_features(..., None, spec, newline=) == map_features(..., img, spec) == img[map_grid_vid], on
    index lists with an empty frame (only its newline rows), a full frame and single tokens."""
    N = h * h
    g = torch.Generator().manual_seed(h)
    sizes = [0, N, 1, max(1, N // 3)]
    F = len(sizes)
    ind = [torch.randperm(N, generator=g)[:k].sort().values for k in sizes]
    x = make_input(F, N, D, dn, 91, "iid")
    nl = newline_vec(D, dn, 92)
    img = img_of(x, nl, F, h)
    spec = dict(MODEL_SPECS["llava_vid"]) if h == 13 else dict(mapper="grid_vid", grid=h, tpf=N)
    indd, xd = [i.to(dev()) for i in ind], x.to(dev())
    old = vc.map_features(indd, xd, img.to(dev()), spec)
    new = vc.map_features(indd, xd, None, spec, newline=nl.to(dev()))
    want = img[O.map_grid_vid(ind, h)]
    same_bits(new, old, "stage API, both routes")
    same_bits(new, want, "stage API against the definition")
    same_bits(new[:h], nl.expand(h, D), "the empty frame: newline rows only")
    same_bits(xd, x, "flat was modified")
    with pytest.raises(ValueError, match="img_feat required for grid mapping"):
        vc.map_features(indd, xd, None, spec)


def test_errors_leave_the_next_call_right():
    F, h, D, dn = 3, 3, 8, "bf16"
    x = make_input(F, h * h, D, dn, 95, "drift")
    nl = newline_vec(D, dn, 96)
    img, ref = reference(x, nl, h, 0.25, dn)
    xd, nld, imgd = x.to(dev()), nl.to(dev()), img.to(dev())

    def valid():
        got = vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=nld)
        assert torch.equal(got.global_idx.cpu(), ref["grid_idx"])
        same_bits(got.rows, img[ref["grid_idx"]], "after an error")

    valid()
    with pytest.raises(ValueError, match="not both"):
        vc.compress(xd, h * h, 0.25, "grid_vid", h, imgd, newline=nld)
    with pytest.raises(ValueError, match="img_feat required for grid mapping"):
        vc.compress(xd, h * h, 0.25, "grid_vid", h)
    with pytest.raises(ValueError, match="grid_vid"):
        vc.compress(xd, h * h, 0.25, "linear", newline=nld)
    valid()
    for bad in (nld.float(), nld[:-1], torch.cat((nld, nld)), nld[None, None], nl, nld.expand(2, D)):
        with pytest.raises(RuntimeError, match="newline must be"):
            vc.compress(xd, h * h, 0.25, "grid_vid", h, newline=bad)
        valid()
    with pytest.raises(RuntimeError, match="grid_vid mapping needs N == grid_h"):      # h * h != N, with a newline
        vc.compress(xd, h * h, 0.25, "grid_vid", 2, newline=nld)
    valid()
    plan = CompressPlan(F, h * h, D, DT[dn], dev(), 0.25, "linear")
    with pytest.raises(ValueError, match="maps linearly"):
        plan.enqueue(xd, newline=nld)
    plan = CompressPlan(F, h * h, D, DT[dn], dev(), 0.25, "grid_vid", h)
    with pytest.raises(ValueError, match="not both"):
        plan.enqueue(xd, imgd, newline=nld)


# ---- the hook ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["video_grid_bf16", "video_grid_f32_r50"])
def test_hook_skips_the_models_method(name, monkeypatch):
    """On the GPU the grid hook does not call the model's add_token_per_grid (0 calls; 1 with VC2_GRID_NEWLINE=off);
    either way the prompt is the golden's, and nothing is left on the instance."""
    from vidcom2_amd.models.llava import cus_prepare_inputs_labels_for_multimodal as hook
    c = next(c for c in load_json("hook_cases.json")["llava"] if c["name"] == name)
    monkeypatch.setenv("R_RATIO", c["r"])
    ids, feats = S.llava_inputs(c)
    ids, feats = ids.to(dev()), feats.to(dev())
    calls = []

    class Counting(S.StubLlava):
        def add_token_per_grid(self, image_feature):
            calls.append(1)
            return super().add_token_per_grid(image_feature)

    for knob, want_calls in ((None, 0), ("on", 0), ("off", 1)):
        if knob is None:
            monkeypatch.delenv("VC2_GRID_NEWLINE", raising=False)
        else:
            monkeypatch.setenv("VC2_GRID_NEWLINE", knob)
        del calls[:]
        m = Counting(c["D"], S.DT[c["dt"]], dev(), c["seed"], c["merge"], c["newline"])
        m.prepare_inputs_labels_for_multimodal = types.MethodType(hook, m)
        comp = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)
        assert len(calls) == want_calls, knob
        assert list(comp[4].shape) == c["comp_shape"] and synth.sha256_tensor(comp[4]) == c["comp_sha"], knob
        assert type(comp[4]) is torch.Tensor
        assert "add_token_per_grid" not in m.__dict__ and "get_2dPool" not in m.__dict__


def test_hook_keeps_the_models_stream_while_a_graph_is_recorded(monkeypatch):
    """A newline (or features) that requires grad with grad enabled: the hook leaves the stream to the model's own
    add_token_per_grid (1 call), so a training step keeps torch's backward of it; under no_grad the same model takes the
    new route (0 calls).  Same prompt either way."""
    from vidcom2_amd.models.llava import cus_prepare_inputs_labels_for_multimodal as hook
    c = next(c for c in load_json("hook_cases.json")["llava"] if c["name"] == "video_grid_bf16")
    monkeypatch.setenv("R_RATIO", c["r"])
    monkeypatch.delenv("VC2_GRID_NEWLINE", raising=False)
    ids, feats = S.llava_inputs(c)
    ids, feats = ids.to(dev()), feats.to(dev())
    calls = []

    class Counting(S.StubLlava):
        def add_token_per_grid(self, image_feature):
            calls.append(1)
            return super().add_token_per_grid(image_feature)

    m = Counting(c["D"], S.DT[c["dt"]], dev(), c["seed"], c["merge"], c["newline"])
    m.model.image_newline.requires_grad_()
    m.prepare_inputs_labels_for_multimodal = types.MethodType(hook, m)
    emb = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)[4]
    assert len(calls) == 1 and emb.requires_grad
    (g,) = torch.autograd.grad(emb, [m.model.image_newline], torch.ones_like(emb))
    assert g.shape == (c["D"],) and float(g.float().sum()) == c["F"] * 13 * c["D"]      # one per newline slot and channel
    del calls[:]
    with torch.no_grad():
        emb2 = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)[4]
    assert len(calls) == 0 and not emb2.requires_grad
    assert synth.sha256_tensor(emb2) == c["comp_sha"] == synth.sha256_tensor(emb.detach())


# ---- autograd ------------------------------------------------------------------------------------------------------
def _grads(F, h, D, dn, g_of):
    """(ours, torch's) gradients of rows with respect to (flattened_feat, newline): ours through compress(newline=),
    torch's through img[global_idx] with img built from leaf tensors by the definition.  g_of(shape) -> upstream gradient."""
    x = make_input(F, h * h, D, dn, 11, "drift").to(dev())
    nl = torch.randn(D, generator=torch.Generator().manual_seed(12)).to(DT[dn]).to(dev())
    xa, na = x.clone().requires_grad_(), nl.clone().requires_grad_()
    res = vc.compress(xa, h * h, 0.25, "grid_vid", h, newline=na)
    assert res.rows.grad_fn is not None and not res.global_idx.requires_grad
    g = g_of(tuple(res.rows.shape)).to(DT[dn]).to(dev())
    ours = torch.autograd.grad(res.rows, [xa, na], g)
    xb, nb = x.clone().requires_grad_(), nl.clone().requires_grad_()
    rows = img_of(xb, nb, F, h)[res.global_idx]
    same_bits(res.rows, rows, "forward")
    theirs = torch.autograd.grad(rows, [xb, nb], g)
    return ours, theirs, g, res


@pytest.mark.parametrize("F,h,D,dn", [(3, 3, 8, "f32"), (3, 13, 64, "bf16"), (2, 13, 6, "f16")])
def test_gradients_equal_torchs(F, h, D, dn):
    """Upstream gradients are small integers (|sum| <= 3 * F * h <= 117: exact in every dtype and summation order), so
    both gradients are bit-equal to torch autograd's."""
    ours, theirs, _, _ = _grads(F, h, D, dn, lambda s: torch.randint(-3, 4, s, generator=torch.Generator().manual_seed(5)).float())
    same_bits(ours[0], theirs[0], "d rows / d flattened_feat")
    same_bits(ours[1], theirs[1], "d rows / d newline")


def test_random_gradients_bf16():
    """Random upstream gradients: flattened_feat's gradient has one term per element (bit-equal); newline's is an
    fp32-accumulated sum rounded once on both sides, in different orders: within one bf16 ulp of the fp64 sum."""
    F, h, D = 3, 13, 64
    ours, theirs, g, res = _grads(F, h, D, "bf16", lambda s: torch.randn(s, generator=torch.Generator().manual_seed(6)))
    same_bits(ours[0], theirs[0], "d rows / d flattened_feat")
    is_nl = res.global_idx % (h + 1) == h
    assert int(is_nl.sum()) == F * h
    exact = g[: res.K][is_nl].double().sum(dim=0).cpu()
    ulp = torch.exp2(torch.floor(torch.log2(exact.abs().clamp_min(2.0 ** -126))) - 7)
    assert ((ours[1].double().cpu() - exact).abs() <= ulp).all()
    assert ((theirs[1].double().cpu() - exact).abs() <= ulp).all()


def test_no_graph_without_grad():
    F, h, D = 2, 3, 8
    x = make_input(F, h * h, D, "f32", 13, "drift").to(dev())
    nl = newline_vec(D, "f32", 14).to(dev())
    assert vc.compress(x, h * h, 0.25, "grid_vid", h, newline=nl).rows.grad_fn is None
    xa, na = x.clone().requires_grad_(), nl.clone().requires_grad_()
    with torch.no_grad():
        r = vc.compress(xa, h * h, 0.25, "grid_vid", h, newline=na).rows
    assert r.grad_fn is None and not r.requires_grad
    only_nl = vc.compress(x, h * h, 0.25, "grid_vid", h, newline=na).rows                # newline alone requires grad
    (gn,) = torch.autograd.grad(only_nl, [na], torch.ones_like(only_nl))
    assert torch.equal(gn.cpu(), torch.full((D,), float(F * h)))

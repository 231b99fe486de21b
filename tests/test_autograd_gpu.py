"""GPU: gradients through the kept-row / kept-column gathers are bit-identical to torch's autograd of the reference
formulas (`flat[global_idx]`, `img[global_idx]`, `x[:, idx]`, `torch.cat`, `inputs_embeds[:, keep]`) on the same kept
indices, and nothing changes where no gradient is wanted."""
import os
import types

import pytest
import torch

import _batched_inputs as BI
import _stub_models as S
import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import fused
from vidcom2_amd.vidcom2 import CompressionResult, _gather_rows, low_var_channel_order

from conftest import DT, make_input

pytestmark = pytest.mark.gpu
DEV = "cuda"
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def bits(t):
    return t.contiguous().view(INT[t.dtype]).cpu()


def same_bits(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    assert torch.equal(bits(a), bits(b))


def grad_out(shape, dtype, seed=0, noncontig=False):
    """Output gradient with +-0.0 elements (torch's backward turns -0.0 into +0.0), optionally a transposed view."""
    g = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)
    g.view(-1)[::7] = -0.0
    g.view(-1)[3::11] = 0.0
    g = g.to(DEV)
    if noncontig:
        g = g.t().contiguous().t()
        assert not g.is_contiguous()
    return g


def torch_grads(fn, inputs, g):
    ins = [t.detach().clone().requires_grad_() for t in inputs]
    return torch.autograd.grad(fn(*ins), ins, g, allow_unused=True)


# ---- compress / vidcom2_compression ----------------------------------------------------------------------------------
CORE = [(1, 196, 512), (3, 50, 72), (4, 49, 64), (6, 64, 128), (6, 196, 256), (8, 196, 1024), (16, 169, 3584)]


def _check_compress(x, tpf, tail=None, noncontig=False, seed=0):
    with torch.no_grad():
        plain = vc.compress(x, tpf, 0.25, tail=tail)
    xg = x.detach().clone().requires_grad_()
    tg = tail.detach().clone().requires_grad_() if tail is not None else None
    res = vc.compress(xg, tpf, 0.25, tail=tg)
    # under grad: the same rows, indices and budgets
    same_bits(res.rows.detach(), plain.rows)
    assert torch.equal(res.global_idx, plain.global_idx) and torch.equal(res.ks, plain.ks) and res.K == plain.K
    assert res.rows.grad_fn is not None and res.global_idx.grad_fn is None
    g = grad_out(tuple(res.rows.shape), x.dtype, seed, noncontig)
    ins = [xg] + ([tg] if tg is not None else [])
    got = torch.autograd.grad(res.rows, ins, g)
    idx = plain.global_idx
    if tail is None:
        ref = torch_grads(lambda a: a[idx], [x], g)
    else:
        ref = torch_grads(lambda a, t: torch.cat((a[idx], t)), [x, tail], g)
    for a, b in zip(got, ref):
        same_bits(a, b)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("shape", CORE, ids=lambda s: "x".join(map(str, s)))
def test_compress_grad_matches_torch_indexing(shape, dt):
    F, N, D = shape
    x = make_input(F, N, D, dt, 3, "drift").to(DEV)
    _check_compress(x, N)
    tail = torch.randn(1, D).to(DT[dt]).to(DEV)
    _check_compress(x, N, tail=tail, noncontig=True, seed=1)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_grid_mapper_grad_goes_to_img_feat_only(dt):
    F, h, D = 4, 13, 256
    dtype = DT[dt]
    x = make_input(F, h * h, D, dt, 5, "drift").to(DEV).requires_grad_()
    img = torch.randn(F * h * (h + 1), D).to(dtype).to(DEV).requires_grad_()
    with torch.no_grad():
        plain = vc.compress(x, h * h, 0.25, "grid_vid", h, img)
    out = vc.vidcom2_compression(x, "llava_vid", img_feat=img)
    same_bits(out.detach(), plain.rows)
    g = grad_out(tuple(out.shape), dtype, 2)
    gx, gimg = torch.autograd.grad(out, [x, img], g, allow_unused=True)
    assert gx is None                                   # (the reference: img[global_idx] does not depend on x)
    same_bits(gimg, torch_grads(lambda a: a[plain.global_idx], [img], g)[0])


@pytest.mark.parametrize("shape,dt", [((4, 196, 5120), "bf16"), ((4, 196, 6144), "f16"),     # D > 4096
                                      ((4, 49, 1000), "f16"), ((4, 49, 1000), "bf16"),         # D % 8 != 0: scalar path
                                      ((3, 50, 1001), "f32")])
def test_compress_grad_wide_and_scalar_rows(shape, dt):
    F, N, D = shape
    x = make_input(F, N, D, dt, 7, "drift").to(DEV)
    _check_compress(x, N, tail=torch.randn(2, D).to(DT[dt]).to(DEV), noncontig=True)


def test_compress_grad_target_shape():
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(128 * 196, 3584, generator=g, device=DEV).to(torch.bfloat16)
    _check_compress(x, 196)


def test_vidcom2_compression_is_differentiable():
    x = make_input(8, 196, 1024, "bf16", 0, "drift").to(DEV).requires_grad_()
    out = vc.vidcom2_compression(x)
    g = grad_out(tuple(out.shape), x.dtype)
    (gx,) = torch.autograd.grad(out, x, g)
    idx = vc.compress(x.detach(), 196).global_idx
    same_bits(gx, torch_grads(lambda a: a[idx], [x], g)[0])


def test_no_graph_without_grad():
    x = make_input(4, 196, 128, "bf16", 1, "drift").to(DEV)
    xg = x.clone().requires_grad_()
    assert vc.vidcom2_compression(x).grad_fn is None
    with torch.no_grad():
        assert vc.vidcom2_compression(xg).grad_fn is None
        assert vc.select_low_var_channels(xg).grad_fn is None
        assert fused.gather_scatter([xg], torch.arange(5, device=DEV))[0].grad_fn is None
    with torch.inference_mode():
        assert vc.vidcom2_compression(xg).grad_fn is None
        assert vc.compress_batch([xg, xg], 196)[0].rows.grad_fn is None
    assert vc.vidcom2_compression(xg).grad_fn is not None


# ---- stage functions and map_features -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,D", [(dt, D) for dt in ("f32", "bf16", "f16") for D in (64, 1000)] +
                         [("bf16", 5120), ("f16", 8192)])
def test_select_low_var_channels_grad(dt, D):
    x = torch.randn(300, D).to(DT[dt]).to(DEV)
    xg = x.clone().requires_grad_()
    out = vc.select_low_var_channels(xg)
    with torch.no_grad():
        same_bits(out.detach(), vc.select_low_var_channels(x))
    idx = low_var_channel_order(x)
    g = grad_out(tuple(out.shape), x.dtype, 4, noncontig=True)
    same_bits(torch.autograd.grad(out, xg, g)[0], torch_grads(lambda a: a[:, idx], [x], g)[0])


@pytest.mark.parametrize("mapper", ["linear", "grid_vid"])
def test_map_features_grad(mapper):
    F, N, D = 4, 169, 256
    flat = torch.randn(F * N, D).to(torch.bfloat16).to(DEV).requires_grad_()
    img = torch.randn(F * 13 * 14, D).to(torch.bfloat16).to(DEV).requires_grad_()
    gen = torch.Generator().manual_seed(0)
    indices = [torch.randperm(N, generator=gen)[:40].sort().values.to(DEV) for _ in range(F)]
    spec = vc.MODEL_SPECS["llava_ov" if mapper == "linear" else "llava_vid"]
    out = vc.map_features(indices, flat, img, spec)
    src = flat if mapper == "linear" else img
    gidx = vc._map_linear_offset(indices, N) if mapper == "linear" else vc._map_grid_vid(indices, 13)
    g = grad_out(tuple(out.shape), out.dtype, 5)
    same_bits(torch.autograd.grad(out, src, g)[0], torch_grads(lambda a: a[gidx], [src], g)[0])


def test_duplicate_indices_fall_back_to_accumulation():
    src = torch.randn(50, 72).to(DEV).requires_grad_()
    idx = torch.tensor([3, 7, 3, 49, 0, 7, 7], device=DEV)
    out = _gather_rows(src, idx)
    g = grad_out(tuple(out.shape), out.dtype, 6)
    torch.testing.assert_close(torch.autograd.grad(out, src, g)[0], torch_grads(lambda a: a[idx], [src], g)[0],
                               rtol=0, atol=0)


# ---- hook-side fusion ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_gather_scatter_three_sources_and_tail(dt):
    dtype = DT[dt]
    srcs = [torch.randn(r, 136).to(dtype).to(DEV).requires_grad_() for r in (400, 400, 300)]
    tail = torch.randn(2, 136).to(dtype).to(DEV).requires_grad_()
    idx = torch.randperm(300, generator=torch.Generator().manual_seed(1))[:120].to(DEV)
    outs = fused.gather_scatter(srcs, idx, tail=tail, check=True)
    gs = [grad_out(tuple(o.shape), dtype, 10 + i, noncontig=i == 1) for i, o in enumerate(outs)]
    got = torch.autograd.grad(outs, srcs + [tail], gs)

    def ref(a, b, c, t):
        return torch.cat((a[idx], t)), b[idx], c[idx]
    ins = [s.detach().clone().requires_grad_() for s in srcs + [tail]]
    want = torch.autograd.grad(ref(*ins), ins, gs)
    for a, b in zip(got, want):
        same_bits(a, b)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_repad_rows_grad_on_a_padded_batch(side, dt):
    c = {**_qwen_case("qwen2_5_vl", 0), "dt": dt}
    rows = BI.row_cases(c, 3)
    ids, feats, grids, mask, lens = BI.batch_inputs(rows, side)
    vm = (ids == S.VIDEO_ID).to(DEV)
    n_video = int(vm.sum())
    kept = torch.randperm(n_video, generator=torch.Generator().manual_seed(2))[: n_video // 3].sort().values.to(DEV)
    lay = fused.keep_positions_batched(vm, kept, n_video, side == "left", attention_mask=mask.to(DEV))
    B, Sfull = ids.shape
    D = c["D"]
    emb = torch.randn(B, Sfull, D).to(DT[dt]).to(DEV)
    eg = emb.clone().requires_grad_()
    out = fused.repad_rows(eg, lay.keep)
    same_bits(out.detach(), fused.repad_rows(emb, lay.keep))
    g = grad_out(tuple(out.shape), emb.dtype, 3)
    keep = lay.keep
    slot = keep >= 0
    flat_idx = (torch.arange(B, device=DEV)[:, None] * Sfull + keep)[slot]
    want = torch_grads(lambda a: a.reshape(B * Sfull, D)[flat_idx], [emb], g[slot])[0]
    same_bits(torch.autograd.grad(out, eg, g)[0], want)


def _qwen_case(family, i):
    import json
    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "hook_cases.json")))[family][i]


# ---- compress_batch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True])
def test_compress_batch_grads_per_clip(mixed):
    shapes = [(6, 64, 128)] * 4 if not mixed else [(6, 64, 128), (4, 49, 128), (8, 64, 128)]
    tpfs = [s[1] for s in shapes]
    clips = [make_input(F, N, D, "bf16", 20 + i, "drift").to(DEV) for i, (F, N, D) in enumerate(shapes)]
    with torch.no_grad():
        plain = vc.compress_batch(clips, tpfs)
    cg = [c.clone().requires_grad_() for c in clips]
    res = vc.compress_batch(cg, tpfs)
    for i, (r, p) in enumerate(zip(res, plain)):
        same_bits(r.rows.detach(), p.rows)
        assert torch.equal(r.global_idx, p.global_idx) and torch.equal(r.ks, p.ks)
        g = grad_out(tuple(r.rows.shape), r.rows.dtype, 30 + i)
        got = torch.autograd.grad(r.rows, cg, g, allow_unused=True, retain_graph=True)
        assert all(got[j] is None for j in range(len(cg)) if j != i)
        same_bits(got[i], torch_grads(lambda a: a[p.global_idx], [clips[i]], g)[0])


# ---- hooks -----------------------------------------------------------------------------------------------------------
def _llava_case(name):
    import json
    from conftest import GOLDEN
    return next(c for c in json.load(open(os.path.join(GOLDEN, "hook_cases.json")))["llava"] if c["name"] == name)


def _torch_compress(flat, tpf, base_scale=0.25, mapper="linear", grid_h=0, img_feat=None, want_scores=False,
                    gather=True, tail=None, stats_ws=None):
    """The reference's compression by torch indexing on the oracle's kept indices."""
    o = O.compress_indices(flat.detach().cpu().contiguous(), tpf, base_scale)
    idx = o["global_idx"]
    if mapper == "grid_vid":
        F = flat.shape[0] // tpf
        loc = idx - torch.repeat_interleave(torch.arange(F) * tpf, o["ks"])
        idx = O.map_grid_vid(list(torch.split(loc, o["ks"].tolist())), grid_h)
    idx = idx.to(flat.device)
    rows = (img_feat if mapper == "grid_vid" else flat)[idx]
    if tail is not None:
        rows = torch.cat((rows, tail.reshape(-1, rows.shape[1])))
    return CompressionResult(rows, idx, o["ks"].to(flat.device), int(idx.numel()))


def _run_llava_grad(c, monkeypatch, reference):
    import vidcom2_amd.models.llava as HL
    import vidcom2_amd.vidcom2 as V
    from vidcom2_amd.models.llava import cus_prepare_inputs_labels_for_multimodal as hook
    monkeypatch.setenv("R_RATIO", c["r"])
    if reference:
        monkeypatch.setattr(V, "compress", _torch_compress)
        monkeypatch.setattr(HL, "vidcom2_compression",
                            lambda flat, model="llava_ov", base_scale=0.25, frame_token_len=None, img_feat=None:
                            _torch_compress(flat, 169 if model == "llava_vid" else 196, base_scale,
                                            "grid_vid" if model == "llava_vid" else "linear", 13, img_feat).rows)
    ids, feats = S.llava_inputs(c)
    m = S.StubLlava(c["D"], S.DT[c["dt"]], DEV, c["seed"], c["merge"], c["newline"])
    m.model.image_newline.requires_grad_()
    feats = feats.to(DEV).requires_grad_()
    m.prepare_inputs_labels_for_multimodal = types.MethodType(hook, m)
    emb = m.prepare_inputs_labels_for_multimodal(ids.to(DEV), None, None, None, None, [feats], ["video"], None)[4]
    g = grad_out(tuple(emb.shape), emb.dtype, 8)
    return emb.detach(), torch.autograd.grad(emb, [feats, m.model.image_newline], g, allow_unused=True)


@pytest.mark.parametrize("name", ["ov_one_token_bf16", "ov_one_token_f16_r15", "video_grid_bf16", "video_grid_f32_r50"])
def test_llava_hook_gradients(name, monkeypatch):
    c = _llava_case(name)
    emb, got = _run_llava_grad(c, monkeypatch, False)
    emb_ref, want = _run_llava_grad(c, monkeypatch, True)
    same_bits(emb, emb_ref)
    for a, b in zip(got, want):
        assert b is not None
        same_bits(a, b)




def _run_qwen_grad(family, c, monkeypatch, reference):
    import vidcom2_amd.models._prefill_prune as PP
    import vidcom2_amd.models.qwen2_5_vl as HQ
    monkeypatch.setenv("R_RATIO", c["r"])
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    if reference:                          # torch indexing on the oracle's kept indices
        monkeypatch.setattr(PP, "_fusable", lambda *a: False)

        def keep(feat, grid, merge, base):
            t, h, w = (int(v) for v in grid.tolist())
            return O.compress_indices(feat.detach().cpu().contiguous(), (h * w) // (merge ** 2), base)["global_idx"].to(DEV)
        monkeypatch.setattr(HQ, "_compute_keep_indices", keep)
    if family == "qwen3_vl":
        from vidcom2_amd.models.qwen3_vl import Qwen3VLModel_forward as hook
    else:
        from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    dtype = S.DT[c["dt"]]
    ids, feats, pos, mask = S.qwen_inputs({**c, "n_image": 0})
    model, rec = S.make_qwen_vl_model(family, c["D"], dtype, DEV, c["seed"])
    rec.embed.weight.requires_grad_()
    feats = [f.to(DEV).requires_grad_() for f in feats]
    n_vid = sum(f.shape[0] for f in feats)
    deep = None
    if family == "qwen3_vl":
        deep = [d.to(DEV).requires_grad_() for d in S.deepstack_feats(n_vid, c["D"], dtype, c["seed"])]
    S.set_video_features(model, feats, deep)
    model.forward = types.MethodType(hook, model)
    model(input_ids=ids.to(DEV), attention_mask=None if mask is None else mask.to(DEV), position_ids=pos.to(DEV),
          pixel_values_videos=torch.zeros(1, 4, device=DEV), video_grid_thw=torch.tensor(c["grids"], device=DEV))
    seen = rec.calls[-1]
    outs = [seen["inputs_embeds"]] + list(seen.get("deepstack_visual_embeds") or [])
    gs = [grad_out(tuple(o.shape), o.dtype, 40 + i) for i, o in enumerate(outs)]
    ins = feats + (deep or []) + [rec.embed.weight]
    return [o.detach() for o in outs], torch.autograd.grad(outs, ins, gs, allow_unused=True)


@pytest.mark.parametrize("family,i", [("qwen2_5_vl", 0), ("qwen2_5_vl", 2), ("qwen3_vl", 0)])
def test_qwen_hook_gradients(family, i, monkeypatch):
    c = _qwen_case(family, i)
    outs, got = _run_qwen_grad(family, c, monkeypatch, False)
    outs_ref, want = _run_qwen_grad(family, c, monkeypatch, True)
    for a, b in zip(outs, outs_ref):
        same_bits(a, b)
    assert got[-1] is not None                         # the text embeddings get their gradient
    for a, b in zip(got, want):
        assert b is not None
        same_bits(a, b)


@pytest.mark.parametrize("mode", ["average", "bilinear", "max"])
def test_fused_pool_backward_is_the_models_pooling_jacobian(mode):
    from vidcom2_amd.models.llava import _fused_pool
    side, D = 27, 128

    def pool_inner(x, stride=2):                       # LLaVA's get_2dPool (llava_arch.py:171-190)
        F = x.shape[0]
        y = x.view(F, side, side, D).permute(0, 3, 1, 2)
        if mode == "average":
            y = torch.nn.functional.avg_pool2d(y, stride)
        elif mode == "max":
            y = torch.nn.functional.max_pool2d(y, stride)
        else:
            y = torch.nn.functional.interpolate(y, size=[(side + 1) // 2] * 2, mode="bilinear")
        return y.permute(0, 2, 3, 1).reshape(F, -1, D)

    model = types.SimpleNamespace(config=types.SimpleNamespace(mm_spatial_pool_mode=mode),
                                  get_vision_tower=lambda: types.SimpleNamespace(num_patches_per_side=side))
    x = torch.randn(4, side * side, D, device=DEV)
    with torch.no_grad():
        plain, _ = _fused_pool(model, pool_inner, x, (), {})
    xg = x.clone().requires_grad_()
    out, ws = _fused_pool(model, pool_inner, xg, (), {})
    same_bits(out.detach(), plain)
    assert ws._vc2_stats_for[4] == out.data_ptr()
    g = torch.randn(out.shape, device=DEV)
    got, want = torch.autograd.grad(out, xg, g)[0], torch_grads(pool_inner, [x], g)[0]
    if mode == "bilinear":      # (torch's bilinear backward accumulates with atomics: its own bits vary run to run)
        torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)
    else:
        same_bits(got, want)

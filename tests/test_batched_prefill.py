"""Batched prefill pruning of the Qwen-VL hooks (`VC2_BATCHED_PREFILL=1`, B > 1 prompts).

The yardstick is the batch-1 hook, pinned to the reference's hook goldens: for every row b, with its own padding removed,
the language model must receive exactly what the batch-1 hook gives that prompt alone.

* `-m "not gpu"`: the hook logic with the CPU oracle standing in for the device pass (as in test_hooks.py) and the
  torch-indexing definition of the batched layout; the real decoder and `generate()`;
* `-m gpu`: the same comparisons through the HIP path (`vc2_keep_positions_batched`, `vc2_repad_rows`).
"""
import os
import types
import warnings

import pytest
import torch

import _batched_inputs as BI
import _stub_models as S
import oracle as O
from conftest import load_json

CASES = load_json("hook_cases.json")
Q25 = {c["name"]: c for c in CASES["qwen2_5_vl"]}
Q3 = {c["name"]: c for c in CASES["qwen3_vl"]}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    O.set_mode("torch")
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    import vidcom2_amd.models._prefill_prune as P
    monkeypatch.setattr(P, "_WARNED", set())


def _oracle_keep(feat, grid, merge, base):
    t, h, w = (int(v) for v in grid.tolist())
    n = (h * w) // (merge ** 2)
    if n <= 0 or feat.numel() == 0:
        return torch.arange(feat.shape[0])
    return O.compress_indices(feat.contiguous().cpu(), n, base)["global_idx"].to(feat.device)


def _use_oracle(monkeypatch):
    import vidcom2_amd.models.qwen2_5_vl as HQ

    def many(feats, grids, merge, base):
        out, off = [], 0
        for f, g in zip(feats, grids):
            out.append(_oracle_keep(f, g, merge, base) + off)
            off += f.shape[0]
        return torch.cat(out) if out else torch.zeros(0, dtype=torch.int64)

    monkeypatch.setattr(HQ, "_compute_keep_indices", _oracle_keep)
    monkeypatch.setattr(HQ, "_compute_keep_indices_many", many)


def _hook(family):
    if family == "qwen3_vl":
        from vidcom2_amd.models.qwen3_vl import Qwen3VLModel_forward
        return Qwen3VLModel_forward
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward
    return Qwen2_5_VLModel_forward


def _pos(mask_or_none, L, B, rows4):
    """Position ids like generate's: text positions of the valid slots (0 at pad slots); 3 planes, or 4 (text + rope
    planes that differ from it)."""
    m = torch.ones((B, L), dtype=torch.int64) if mask_or_none is None else mask_or_none
    t = BI.text_positions(m)
    if not rows4:
        return t[None].expand(3, B, L).contiguous()
    return torch.cat((t[None], torch.where(m != 0, t * 2 + 1, torch.zeros((), dtype=torch.int64))[None].expand(3, B, L)))


def _run(family, c, ids, feats, grids, mask, pos, device, deep=None, cache_position=None):
    dtype = S.DT[c["dt"]]
    model, rec = S.make_qwen_vl_model(family, c["D"], dtype, device, c["seed"])
    S.set_video_features(model, [f.to(device) for f in feats], None if deep is None else [d.to(device) for d in deep])
    model.forward = types.MethodType(_hook(family), model)
    kw = dict(input_ids=ids.to(device), attention_mask=None if mask is None else mask.to(device),
              position_ids=pos.to(device))
    if grids:
        kw.update(pixel_values_videos=torch.zeros(1, 4, device=device), video_grid_thw=torch.tensor(grids, device=device))
    if cache_position is not None:
        kw["cache_position"] = cache_position.to(device)
    model(**kw)
    return model, rec.calls[-1]


def _deep_for(c, n):
    return S.deepstack_feats(n, c["D"], S.DT[c["dt"]], c["seed"] + 77)


def _check_batch(family, c, rows, side, device, rows4=False):
    """Run the batch and every row alone; compare what the language model receives, row by row."""
    if side == "none":
        ids, feats, grids, mask, lens = BI.batch_inputs(rows, "left")
        assert len(set(lens)) == 1
        mask = None
    else:
        ids, feats, grids, mask, lens = BI.batch_inputs(rows, side)
    B, L = ids.shape
    n_vid = sum(f.shape[0] for f in feats)
    deep = _deep_for(c, n_vid) if family == "qwen3_vl" else None
    model, seen = _run(family, c, ids, feats, grids, mask, _pos(mask, L, B, rows4), device, deep, torch.arange(L))
    st = model._vidcom2_last
    assert st.pruned
    keep = st.keep_token_indices
    Sp = seen["inputs_embeds"].shape[1]
    assert keep.shape == (B, Sp) and st.lengths.tolist() == (keep >= 0).sum(1).tolist()
    assert Sp == int(st.lengths.max()) <= L and int(st.lengths.min()) < L
    am = seen["attention_mask"]
    assert am.shape == (B, Sp) and seen["cache_position"].tolist() == list(range(Sp))
    pos = seen["position_ids"]
    assert pos.shape == ((4 if rows4 else 3), B, Sp)
    vid_off, deep_rows = 0, []
    for b, r in enumerate(rows):
        rid, rfeats, rgrids = BI.single_inputs(r)
        n = rid.shape[1]
        nv = sum(f.shape[0] for f in rfeats)
        rdeep = [d[vid_off:vid_off + nv] for d in deep] if deep is not None and nv else None
        rmask = None if mask is None else torch.ones((1, n), dtype=torch.int64)
        one_model, one = _run(family, c, rid, rfeats, rgrids, rmask, _pos(rmask, n, 1, rows4), device, rdeep)
        vid_off += nv
        m = one["inputs_embeds"].shape[1]
        valid = (am[b] != 0).cpu()
        assert int(valid.sum()) == m
        sl = slice(Sp - m, Sp) if side in ("left", "none") else slice(0, m)
        assert valid[sl].all()
        assert torch.equal(seen["inputs_embeds"][b, sl].cpu(), one["inputs_embeds"][0].cpu())
        assert torch.equal(pos[:, b, sl].cpu(), one["position_ids"][:, 0].cpu())
        if rgrids:
            shift = L - n if side == "left" else 0                 # (the row's own left padding)
            assert torch.equal(keep[b, sl].cpu() - shift, one_model._vidcom2_last.keep_token_indices.cpu())
        # pad slots: masked, the pad position value (0 for these inputs), and new ones zero rows
        pad = ~valid
        assert (pos[:, b][:, pad.to(pos.device)] == 0).all()
        new_pad = (keep[b] < 0).cpu()
        assert (seen["inputs_embeds"][b][new_pad.to(seen["inputs_embeds"].device)] == 0).all()
        if family == "qwen3_vl":
            vpm = seen["visual_pos_masks"]
            if rgrids:
                assert torch.equal(vpm[b, sl].cpu(), one["visual_pos_masks"][0].cpu())
                deep_rows.append(one["deepstack_visual_embeds"])
            assert not vpm[b][pad.to(vpm.device)].any()
    if family == "qwen3_vl":
        for l, d in enumerate(seen["deepstack_visual_embeds"]):
            assert torch.equal(d.cpu(), torch.cat([dr[l].cpu() for dr in deep_rows]))
    return model, seen


# ------------------------------------------------------------------------------------------
# CPU: hook logic (oracle for the device pass, torch-indexing layout)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("n_rows", [2, 3, 4])
@pytest.mark.parametrize("name", ["one_video_bf16", "two_videos_f32_r50_4dmask"])
def test_batched_equals_per_sample_qwen25_cpu(name, n_rows, side, monkeypatch):
    _use_oracle(monkeypatch)
    c = Q25[name]
    monkeypatch.setenv("R_RATIO", c["r"])
    _check_batch("qwen2_5_vl", c, BI.row_cases(c, n_rows), side, "cpu")


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", ["video_only_bf16", "image_and_two_videos_f32"])
def test_batched_equals_per_sample_qwen3_cpu(name, side, monkeypatch):
    _use_oracle(monkeypatch)
    c = Q3[name]
    monkeypatch.setenv("R_RATIO", c["r"])
    _check_batch("qwen3_vl", c, BI.row_cases(c, 3), side, "cpu")


def _same_length_rows(c):
    a = dict(c, n_image=0)
    b = dict(a, seed=c["seed"] + 500, prefix=c["prefix"] + 2, suffix=c["suffix"] - 2)
    return [a, b]


@pytest.mark.parametrize("family,name", [("qwen2_5_vl", "two_videos_f32_r50_4dmask"), ("qwen3_vl", "video_only_bf16")])
def test_batched_no_mask_creates_one_cpu(family, name, monkeypatch):
    _use_oracle(monkeypatch)
    c = (Q25 if family == "qwen2_5_vl" else Q3)[name]
    monkeypatch.setenv("R_RATIO", c["r"])
    _, seen = _check_batch(family, c, _same_length_rows(c), "none", "cpu")
    assert seen["attention_mask"].dim() == 2


def test_batched_four_row_positions_cpu(monkeypatch):
    _use_oracle(monkeypatch)
    c = Q25["one_video_bf16"]
    monkeypatch.setenv("R_RATIO", c["r"])
    for side in ("left", "right"):
        _check_batch("qwen2_5_vl", c, BI.row_cases(c, 3), side, "cpu", rows4=True)


def test_batched_layout_pad_values_from_existing_pad_slots():
    """New pad slots take the row's own pad position value (its first existing pad slot), 0 when the row has none."""
    from vidcom2_amd.models._prefill_prune import _batched_layout
    vm = torch.tensor([[0, 0, 1, 1, 1, 0], [0, 1, 1, 0, 0, 0]], dtype=torch.bool)
    am = torch.tensor([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    pos = torch.arange(12).view(1, 2, 6).repeat(2, 1, 1) + 100
    pos[:, 0, 0] = 7
    lay = _batched_layout(vm, torch.tensor([1, 3]), True, am, pos, text_row0=True)
    # row 0 keeps 0, 1, 3, 5 (video ordinal 1 of 0..2); row 1 keeps its first video token (ordinal 3), drops position 2
    assert lay.keep.tolist() == [[-1, 0, 1, 3, 5], [0, 1, 3, 4, 5]]
    assert lay.lengths.tolist() == [4, 5]
    assert lay.mask.tolist() == [[0, 0, 1, 1, 1], [1, 1, 1, 1, 1]]
    assert lay.pos[1].tolist() == [[7, 7, 101, 103, 105], [106, 107, 109, 110, 111]]
    assert lay.pos[0].tolist() == [[7, 7, 0, 1, 2], [0, 1, 2, 3, 4]]
    right = _batched_layout(vm, torch.tensor([1, 3]), False, am, pos)
    assert right.keep.tolist() == [[0, 1, 3, 5, -1], [0, 1, 3, 4, 5]]
    assert right.pos[0, 0].tolist() == [7, 101, 103, 105, 7]


# ------------------------------------------------------------------------------------------
# gating
# ------------------------------------------------------------------------------------------
def _two_rows(c):
    return BI.batch_inputs(BI.row_cases(c, 2, with_empty=False), "left")


def test_knob_unset_leaves_the_batch_alone(monkeypatch):
    _use_oracle(monkeypatch)
    monkeypatch.delenv("VC2_BATCHED_PREFILL")
    c = Q25["one_video_bf16"]
    ids, feats, grids, mask, _ = _two_rows(c)
    model, seen = _run("qwen2_5_vl", c, ids, feats, grids, mask, _pos(mask, ids.shape[1], 2, False), "cpu")
    assert seen["inputs_embeds"].shape[:2] == ids.shape
    assert not model._vidcom2_last.pruned


def test_four_d_mask_runs_unpruned_with_one_warning(monkeypatch):
    _use_oracle(monkeypatch)
    c = Q25["one_video_bf16"]
    ids, feats, grids, mask, _ = _two_rows(c)
    L = ids.shape[1]
    m4 = torch.triu(torch.full((L, L), float("-inf")), diagonal=1)[None, None].expand(2, 1, L, L).to(torch.bfloat16)
    with pytest.warns(RuntimeWarning, match="unpruned") as rec:
        model, seen = _run("qwen2_5_vl", c, ids, feats, grids, m4, _pos(None, L, 2, False), "cpu")
        _run("qwen2_5_vl", c, ids, feats, grids, m4, _pos(None, L, 2, False), "cpu")
    assert len([w for w in rec if "unpruned" in str(w.message)]) == 1
    assert seen["inputs_embeds"].shape[:2] == ids.shape and not model._vidcom2_last.pruned
    assert seen["attention_mask"] is not None and seen["attention_mask"].dim() == 4


def test_mixed_padding_runs_unpruned(monkeypatch):
    _use_oracle(monkeypatch)
    c = Q25["one_video_bf16"]
    ids, feats, grids, mask, _ = _two_rows(c)
    mask = mask.clone()
    mask[0, -1] = 0
    mask[0, 0] = 0
    with pytest.warns(RuntimeWarning, match="neither left- nor right-padded"):
        model, seen = _run("qwen2_5_vl", c, ids, feats, grids, mask, _pos(mask, ids.shape[1], 2, False), "cpu")
    assert seen["inputs_embeds"].shape[:2] == ids.shape and not model._vidcom2_last.pruned


def test_batch_of_one_takes_todays_path(monkeypatch):
    """B = 1 with the knob set: the batch-1 path, 1-D keep list as before."""
    _use_oracle(monkeypatch)
    c = Q25["one_video_bf16"]
    monkeypatch.setenv("R_RATIO", c["r"])
    ids, feats, pos, mask = S.qwen_inputs(c)
    model, seen = _run("qwen2_5_vl", c, ids, feats, c["grids"], mask, pos, "cpu")
    assert model._vidcom2_last.keep_token_indices.tolist() == c["keep_token_indices"]
    assert seen["position_ids"][0, 0].tolist() == c["keep_token_indices"]


# ------------------------------------------------------------------------------------------
# real decoder and generate()
# ------------------------------------------------------------------------------------------
D = 64


def _real_model(cls_name="Qwen2_5_VLModel"):
    from transformers.models.qwen2_5_vl import Qwen2_5_VLConfig
    from transformers.models.qwen2_5_vl import modeling_qwen2_5_vl as M
    vision = dict(depth=1, hidden_size=32, intermediate_size=32, num_heads=2, out_hidden_size=D,
                  fullatt_block_indexes=[0], spatial_merge_size=2)
    text = dict(vocab_size=S.VOCAB, hidden_size=D, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                num_key_value_heads=2, max_position_embeddings=4096, bos_token_id=1, eos_token_id=2, pad_token_id=0,
                rope_parameters=dict(rope_type="default", mrope_section=[4, 6, 6], rope_theta=10000.0))
    cfg = Qwen2_5_VLConfig(text_config=text, vision_config=vision, image_token_id=S.IMAGE_ID, video_token_id=S.VIDEO_ID)
    torch.manual_seed(0)
    return getattr(M, cls_name)(cfg).eval()


_REAL = dict(D=D, dt="f32", seed=22, r="0.5", grids=[[4, 8, 8], [6, 12, 8]], prefix=7, between=3, suffix=5, mask="2d",
             n_image=0)


@pytest.mark.parametrize("side", ["left", "right"])
@torch.no_grad()
def test_batched_real_decoder_equals_rows_alone(side, monkeypatch):
    _use_oracle(monkeypatch)
    monkeypatch.setenv("R_RATIO", _REAL["r"])
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    rows = BI.row_cases(_REAL, 3)
    ids, feats, grids, mask, lens = BI.batch_inputs(rows, side)
    model = _real_model()
    model.forward = types.MethodType(hook, model)
    S.set_video_features(model, feats)
    out = model(input_ids=ids, attention_mask=mask, pixel_values_videos=torch.zeros(1, 4),
                video_grid_thw=torch.tensor(grids), mm_token_type_ids=(ids == S.VIDEO_ID).int() * 2).last_hidden_state
    st = model._vidcom2_last
    assert st.pruned and out.shape[1] == st.keep_token_indices.shape[1] <= ids.shape[1]
    for b, r in enumerate(rows):
        rid, rfeats, rgrids = BI.single_inputs(r)
        S.set_video_features(model, rfeats)
        kw = dict(input_ids=rid, attention_mask=torch.ones_like(rid), mm_token_type_ids=(rid == S.VIDEO_ID).int() * 2)
        if rgrids:
            kw.update(pixel_values_videos=torch.zeros(1, 4), video_grid_thw=torch.tensor(rgrids))
        one = model(**kw).last_hidden_state
        m = one.shape[1]
        sl = slice(out.shape[1] - m, out.shape[1]) if side == "left" else slice(0, m)
        assert torch.allclose(out[b, sl], one[0], atol=1e-5)


def _margins_ok(logits):
    for step in logits:
        top = step.float().topk(2, dim=-1).values
        assert ((top[:, 0] - top[:, 1]) > 1e-3).all(), "top-2 logits too close for token equality to mean anything"


@torch.no_grad()
def test_generate_left_padded_batch_equals_samples_alone(monkeypatch):
    _use_oracle(monkeypatch)
    monkeypatch.setenv("R_RATIO", _REAL["r"])
    from vidcom2_amd.models import install
    model = _real_model("Qwen2_5_VLForConditionalGeneration")
    assert install(model)
    rows = BI.row_cases(_REAL, 2, with_empty=False)
    rows[1] = dict(rows[1], prefix=rows[1]["prefix"] + 6)          # (different lengths: real left padding)
    ids, feats, grids, mask, lens = BI.batch_inputs(rows, "left")
    assert len(set(lens)) == 2
    gen = dict(max_new_tokens=3, do_sample=False, eos_token_id=None, pad_token_id=0, output_logits=True,
               return_dict_in_generate=True)
    S.set_video_features(model.model, feats)
    out = model.generate(input_ids=ids, attention_mask=mask, pixel_values_videos=torch.zeros(1, 4),
                         video_grid_thw=torch.tensor(grids), mm_token_type_ids=(ids == S.VIDEO_ID).int() * 2, **gen)
    assert model.model._vidcom2_last.pruned and model.model._vidcom2_last.keep_token_indices.shape[0] == 2
    _margins_ok(out.logits)
    for b, r in enumerate(rows):
        rid, rfeats, rgrids = BI.single_inputs(r)
        S.set_video_features(model.model, rfeats)
        one = model.generate(input_ids=rid, attention_mask=torch.ones_like(rid), pixel_values_videos=torch.zeros(1, 4),
                             video_grid_thw=torch.tensor(rgrids), mm_token_type_ids=(rid == S.VIDEO_ID).int() * 2, **gen)
        assert model.model._vidcom2_last.pruned
        _margins_ok(one.logits)
        for step, (lb, l1) in enumerate(zip(out.logits, one.logits)):
            assert torch.allclose(lb[b], l1[0], atol=1e-4), step
        assert out.sequences[b, ids.shape[1]:].tolist() == one.sequences[0, rid.shape[1]:].tolist()


def test_decode_mask_mapping_forms():
    """The decode-step mask generate hands over (2-D, 4-D, dict, none) is mapped onto the pruned layout."""
    from vidcom2_amd.models._prefill_prune import _DecodeLayout, _map_decode_mask
    keep = torch.tensor([[-1, 0, 2], [0, 1, 3]])
    dec = _DecodeLayout(torch.tensor([[0, 1, 1], [1, 1, 1]]), keep, 4)
    am = torch.tensor([[1, 1, 0, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    assert _map_decode_mask(am, dec, 4, 1, 2).tolist() == [[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]
    assert _map_decode_mask(None, dec, 4, 1, 2).tolist() == [[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]
    m4 = torch.arange(12, dtype=torch.float32).view(2, 1, 1, 6)
    got = _map_decode_mask(m4, dec, 4, 1, 2)
    lo = torch.finfo(torch.float32).min
    assert got.view(2, 5).tolist() == [[lo, 0, 2, 4, 5], [6, 7, 9, 10, 11]]
    d = _map_decode_mask({"full_attention": am}, dec, 4, 1, 2)
    assert d["full_attention"].tolist() == [[0, 1, 1, 1, 1], [1, 1, 1, 1, 1]]


# ------------------------------------------------------------------------------------------
# GPU: the HIP path, bit-equal per row to the GPU batch-1 hook
# ------------------------------------------------------------------------------------------
def _as(c, dt):
    return dict(c, dt=dt)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("side", ["left", "right", "none"])
@pytest.mark.parametrize("name", ["one_video_bf16", "two_videos_f32_r50_4dmask", "one_video_f16_r10"])
def test_batched_hook_gpu_qwen25(name, side, dt, monkeypatch):
    c = _as(Q25[name], dt)
    monkeypatch.setenv("R_RATIO", c["r"])
    rows = _same_length_rows(c) if side == "none" else BI.row_cases(c, 3)
    _check_batch("qwen2_5_vl", c, rows, side, "cuda", rows4=(name == "one_video_bf16"))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("name", ["video_only_bf16", "image_and_two_videos_f32"])
def test_batched_hook_gpu_qwen3(name, side, dt, monkeypatch):
    c = _as(Q3[name], dt)
    monkeypatch.setenv("R_RATIO", c["r"])
    _check_batch("qwen3_vl", c, BI.row_cases(c, 3), side, "cuda")


@pytest.mark.gpu
def test_batched_hook_gpu_takes_the_device_path(monkeypatch):
    """The batch is pruned by the HIP kernels, not by the torch-indexing definition."""
    import vidcom2_amd.models._prefill_prune as P
    monkeypatch.setattr(P, "_batched_layout", None)
    c = Q25["one_video_bf16"]
    monkeypatch.setenv("R_RATIO", c["r"])
    _check_batch("qwen2_5_vl", c, BI.row_cases(c, 2), "left", "cuda")

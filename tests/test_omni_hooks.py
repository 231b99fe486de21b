"""Qwen2.5-Omni and Qwen3-Omni thinker hooks (`vidcom2_amd.models.qwen2_5_omni` / `qwen3_omni`).

Tiny random-weight thinkers of the installed transformers (`_omni_models.py`).  The yardstick is a by-hand restatement
of the pruned prefill: per-video keep indices, every non-video token kept, the thinker's TMRoPE positions of the
UNPRUNED prompt sliced, attention mask and labels cut -- and, for generation, decode steps continuing at the unpruned
prompt's positions (`S + t + rope_deltas`).

* `-m "not gpu"`: the device pass is replaced by the CPU oracle (as in test_hooks_real_decoder.py);
* `-m gpu`: keep indices from `vidcom2_amd.compress`, the prompt cut by the fused kernels.
"""
import copy
import types
import warnings

import pytest
import torch

import _omni_models as OM
import _stub_models as S
import oracle as O

FAMILIES = ["qwen2_5_omni", "qwen3_omni"]
R = 0.5


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    O.set_mode("torch")
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", str(R))
    monkeypatch.delenv("VC2_BATCHED_PREFILL", raising=False)
    import vidcom2_amd.models._prefill_prune as P
    monkeypatch.setattr(P, "_WARNED", set())


def _oracle_keep(feat, grid, merge, base):
    t, h, w = (int(v) for v in grid.tolist())
    return O.compress_indices(feat.contiguous().float().cpu() if feat.dtype == torch.float32 else
                              feat.contiguous().cpu(), (h * w) // (merge ** 2), base)["global_idx"].to(feat.device)


@pytest.fixture()
def oracle_pass(monkeypatch):
    import vidcom2_amd.models.qwen2_5_vl as HQ

    def many(feats, grids, merge, base):
        out, off = [], 0
        for f, g in zip(feats, grids):
            out.append(_oracle_keep(f, g, merge, base) + off)
            off += f.shape[0]
        return torch.cat(out)

    monkeypatch.setattr(HQ, "_compute_keep_indices", _oracle_keep)
    monkeypatch.setattr(HQ, "_compute_keep_indices_many", many)


def _hook(family):
    if family == "qwen3_omni":
        from vidcom2_amd.models.qwen3_omni import Qwen3OmniMoeThinker_forward
        return Qwen3OmniMoeThinker_forward
    from vidcom2_amd.models.qwen2_5_omni import Qwen2_5OmniThinker_forward
    return Qwen2_5OmniThinker_forward


def _record(model):
    """Keyword arguments of every call into the thinker's decoder stack."""
    calls = []
    model.model.register_forward_pre_hook(lambda mod, args, kw: calls.append(dict(kw)), with_kwargs=True)
    return calls


def _keep_by_hand(p, keep_fn=_oracle_keep):
    """(kept video ordinals, kept positions) of a batch-1 prompt: each video scored alone, every other token kept."""
    ids = p["ids"][0]
    kept, off = [], 0
    for f, g in zip(p["video"], p["kw"]["video_grid_thw"]):
        kept.append(keep_fn(f, g, 2, R).cpu() + off)
        off += f.shape[0]
    kept = torch.cat(kept)
    vm = ids == S.VIDEO_ID
    flags = ~vm
    flags[vm.nonzero().squeeze(-1)[kept]] = True
    return kept, flags.nonzero().squeeze(-1)


def _embeds(model, p):
    """The thinker's prompt embeddings with every modality scattered in (what it hands its decoder, unpruned)."""
    dev = next(model.parameters()).device
    ids = p["ids"].to(dev)
    emb = model.get_input_embeddings()(ids).clone()
    if p["audio"] is not None:
        emb[ids == OM.AUDIO_ID] = p["audio"].to(dev, emb.dtype)
    if p["image"]:
        emb[ids == S.IMAGE_ID] = torch.cat(p["image"]).to(dev, emb.dtype)
    emb[ids == S.VIDEO_ID] = torch.cat(p["video"]).to(dev, emb.dtype)
    return emb


def _positions(model, p):
    """TMRoPE positions and rope deltas of the UNPRUNED prompt, from the thinker's own `get_rope_index`."""
    kw = p["kw"]
    fam = kw.get("feature_attention_mask")
    pos, deltas = model.get_rope_index(kw["input_ids"], kw.get("image_grid_thw"), kw.get("video_grid_thw"),
                                       kw["attention_mask"], kw["use_audio_in_video"],
                                       None if fam is None else fam.sum(1), kw.get("video_second_per_grid"))
    return pos, deltas


def _deep_by_hand(p, keep):
    """Qwen3-Omni deep-stack rows: visual positions (image + video) in prompt order, kept ones only."""
    ids = p["ids"][0]
    vis = (ids == S.VIDEO_ID) | (ids == S.IMAGE_ID)
    flags = torch.zeros(ids.shape[0], dtype=torch.bool)
    flags[keep] = True
    out = []
    for l, dv in enumerate(p["deep"]["video"]):
        joint = dv.new_zeros(int(vis.sum()), dv.shape[1])
        joint[(ids == S.VIDEO_ID)[vis]] = dv
        if p["deep"]["image"] is not None:
            joint[(ids == S.IMAGE_ID)[vis]] = p["deep"]["image"][l]
        out.append(joint[flags[vis]])
    return vis[keep][None], out


def _check_decoder_inputs(family, model, p, seen, keep):
    dev = seen["inputs_embeds"].device
    pos, _ = _positions(model, p)
    assert torch.equal(seen["inputs_embeds"], _embeds(model, p)[:, keep.to(dev)])
    assert torch.equal(seen["position_ids"].cpu(), pos[..., keep].cpu())
    assert torch.equal(seen["attention_mask"].cpu(), p["kw"]["attention_mask"].cpu()[:, keep])
    if family == "qwen3_omni":
        vpm, deep = _deep_by_hand(p, keep)
        assert torch.equal(seen["visual_pos_masks"].cpu(), vpm)
        assert len(seen["deepstack_visual_embeds"]) == len(deep)
        for got, want in zip(seen["deepstack_visual_embeds"], deep):
            assert torch.equal(got.cpu(), want)


PROMPTS = {
    "two_videos": dict(grids=[[4, 8, 8], [3, 4, 8]]),
    "image_and_two_videos": dict(grids=[[4, 8, 8], [3, 4, 8]], n_image_grid=[1, 4, 4]),
    "one_video": dict(grids=[[6, 8, 8]]),
}


def _prompt(family, name, audio_in_video, seed=5, dtype=torch.float32):
    return OM.prompt(family, seed=seed, audio_in_video=audio_in_video, dtype=dtype,
                     deep_layers=2 if family == "qwen3_omni" else 0, **PROMPTS[name])


# ------------------------------------------------------------------------------------------
# install()
# ------------------------------------------------------------------------------------------
def _outer(family, talker=False):
    th = OM.thinker(family)
    if family == "qwen3_omni":
        from transformers.models.qwen3_omni_moe import Qwen3OmniMoeConfig as Cfg
        from transformers.models.qwen3_omni_moe import Qwen3OmniMoeForConditionalGeneration as Model
    else:
        from transformers.models.qwen2_5_omni import Qwen2_5OmniConfig as Cfg
        from transformers.models.qwen2_5_omni import Qwen2_5OmniForConditionalGeneration as Model
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = Model(Cfg(thinker_config=th.config.to_dict(), enable_audio_output=False)).eval()
    if talker:          # what the outer generate reads before it calls the thinker (the talker itself never runs here)
        model.has_talker = True
        model.talker = types.SimpleNamespace(codec_pad_token=0)
        if family == "qwen3_omni":
            model.config.talker_config.speaker_id = {"ethan": 0}
        else:
            model.speaker_map["Chelsie"] = {}
    return model


@pytest.mark.parametrize("family", FAMILIES)
def test_install_binds_on_outer_model_and_thinker(family):
    from vidcom2_amd.models import install
    th = OM.thinker(family)
    assert install(th)
    assert th.__dict__["forward"].__func__ is _hook(family)
    outer = _outer(family)
    assert install(outer)
    assert outer.thinker.__dict__["forward"].__func__ is _hook(family)
    assert "generate" in outer.__dict__ and "forward" not in outer.__dict__


# ------------------------------------------------------------------------------------------
# CPU: decoder inputs, labels, generation, batches, gating (oracle for the device pass)
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("audio_in_video", [False, True], ids=["separate_audio", "audio_in_video"])
@pytest.mark.parametrize("name", ["two_videos", "image_and_two_videos"])
@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_hooked_decoder_inputs_equal_restatement(family, name, audio_in_video, oracle_pass):
    model = OM.thinker(family)
    p = _prompt(family, name, audio_in_video)
    OM.set_features(model, p)
    model.forward = types.MethodType(_hook(family), model)
    calls = _record(model)
    labels = p["ids"].clone()
    out = model(**p["kw"], labels=labels)
    st = model._vidcom2_last
    kept, keep = _keep_by_hand(p)
    assert st.pruned and torch.equal(st.kept_video, kept) and torch.equal(st.keep_token_indices, keep)
    ids = p["ids"][0]
    assert (ids[keep] != S.VIDEO_ID).sum() == (ids != S.VIDEO_ID).sum()          # text, image, audio all kept
    if audio_in_video:
        assert int((ids == OM.AUDIO_ID).sum()) > 0
        vpos = (ids == S.VIDEO_ID).nonzero().squeeze(-1)
        assert (vpos.diff() > 1).any()                                            # audio interleaved with frames
    _check_decoder_inputs(family, model, p, calls[-1], keep)
    assert out.logits.shape[1] == keep.numel() < ids.numel()
    want = model.loss_function(logits=out.logits, labels=labels[:, keep], vocab_size=S.VOCAB)
    assert torch.equal(out.loss, want)


@pytest.mark.parametrize("family", FAMILIES)
def test_labels_loss_backpropagates(family, oracle_pass):
    model = OM.thinker(family)
    p = _prompt(family, "one_video", True)
    OM.set_features(model, p)
    model.forward = types.MethodType(_hook(family), model)
    out = model(**p["kw"], labels=p["ids"].clone())
    out.loss.backward()
    assert model.lm_head.weight.grad is not None and model.lm_head.weight.grad.abs().sum() > 0


def _margins_ok(logits):
    for step in logits:
        top = step.float().topk(2, dim=-1).values
        assert ((top[:, 0] - top[:, 1]) > 1e-3).all(), "top-2 logits too close for token equality to mean anything"


@pytest.mark.parametrize("audio_in_video", [False, True], ids=["separate_audio", "audio_in_video"])
@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_generate_continues_at_unpruned_positions(family, audio_in_video, oracle_pass):
    """Greedy generate through the hooked thinker == a manual prefill on the pruned prompt followed by decode steps at
    positions S + t + rope_deltas of the UNPRUNED prompt."""
    from transformers import DynamicCache
    model = OM.thinker(family)
    p = _prompt(family, "two_videos", audio_in_video)
    OM.set_features(model, p)
    model.forward = types.MethodType(_hook(family), model)
    n_new = 4
    gen = model.generate(**p["kw"], max_new_tokens=n_new, do_sample=False, eos_token_id=None, pad_token_id=0,
                         output_logits=True, return_dict_in_generate=True)
    _, keep = _keep_by_hand(p)
    assert model._vidcom2_last.pruned and torch.equal(model._vidcom2_last.keep_token_indices, keep)
    Sfull = p["ids"].shape[1]
    pos, deltas = _positions(model, p)
    emb = _embeds(model, p)
    cache = DynamicCache(config=model.config.get_text_config())
    deep = {}
    if family == "qwen3_omni":
        vpm, ds = _deep_by_hand(p, keep)
        deep = dict(visual_pos_masks=vpm, deepstack_visual_embeds=ds)
    h = model.model(inputs_embeds=emb[:, keep], position_ids=pos[..., keep], attention_mask=p["kw"]["attention_mask"][:,
                    keep], past_key_values=cache, use_cache=True, **deep).last_hidden_state
    logits = [model.lm_head(h[:, -1])]
    tokens = [int(logits[-1].argmax(-1))]
    for t in range(1, n_new):
        step = (torch.tensor(Sfull + t - 1) + deltas).to(pos.dtype).view(1, 1, 1).expand(3, 1, 1)
        h = model.model(inputs_embeds=model.get_input_embeddings()(torch.tensor([[tokens[-1]]])), position_ids=step,
                        attention_mask=torch.ones(1, keep.numel() + t, dtype=torch.int64), past_key_values=cache,
                        use_cache=True).last_hidden_state
        logits.append(model.lm_head(h[:, -1]))
        tokens.append(int(logits[-1].argmax(-1)))
    _margins_ok(gen.logits)
    assert gen.sequences[0, Sfull:].tolist() == tokens
    for a, b in zip(gen.logits, logits):
        assert torch.allclose(a, b, atol=1e-4, rtol=0)


def _batch(family, side, audio_in_video, dtype=torch.float32):
    """Three prompts of different lengths (two videos / one video / text only), padded on `side`, and the rows."""
    specs = [dict(grids=[[4, 8, 8], [3, 4, 8]], prefix=5), dict(grids=[[6, 8, 8]], prefix=9), dict(grids=[], prefix=7)]
    rows = [OM.prompt(family, seed=5 + 10 * i, audio_in_video=audio_in_video, dtype=dtype,
                      deep_layers=2 if family == "qwen3_omni" else 0, **s) for i, s in enumerate(specs)]
    L = max(r["ids"].shape[1] for r in rows)
    B = len(rows)
    ids = torch.zeros(B, L, dtype=torch.int64)
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b, r in enumerate(rows):
        n = r["ids"].shape[1]
        sl = slice(L - n, L) if side == "left" else slice(0, n)
        ids[b, sl], mask[b, sl] = r["ids"][0], 1
    grids = [g for r in rows for g in r["kw"].get("video_grid_thw", torch.zeros(0, 3, dtype=torch.int64)).tolist()]
    kw = dict(input_ids=ids, attention_mask=mask, use_audio_in_video=audio_in_video,
              pixel_values_videos=torch.zeros(1, 4), video_grid_thw=torch.tensor(grids),
              video_second_per_grid=torch.ones(len(grids)))
    audio = [r["audio"] for r in rows if r["audio"] is not None]
    if audio:
        kw.update(input_features=torch.cat([r["kw"]["input_features"] for r in rows if r["audio"] is not None]),
                  feature_attention_mask=torch.cat([r["kw"]["feature_attention_mask"] for r in rows
                                                    if r["audio"] is not None]))
    merged = dict(ids=ids, video=[f for r in rows for f in r["video"]], image=[],
                  audio=torch.cat(audio) if audio else None, kw=kw, deep=None)
    if family == "qwen3_omni":
        merged["deep"] = dict(video=[torch.cat([r["deep"]["video"][l] for r in rows]) for l in range(2)], image=None)
    return merged, rows


def _check_rows(model, merged, rows, side, calls, out, atol=1e-5):
    """Row by row, the batch's decoder inputs and outputs == the row's own pruned prefill."""
    st = model._vidcom2_last
    assert st.pruned
    seen = calls[-1]
    Sp = seen["inputs_embeds"].shape[1]
    assert st.keep_token_indices.shape == (len(rows), Sp)
    for b, r in enumerate(rows):
        OM.set_features(model, r)
        one_kw = OM.to_device(r["kw"], next(model.parameters()).device)
        one = model(**one_kw)
        m = one.logits.shape[1]
        alone = calls[-1]
        sl = slice(Sp - m, Sp) if side == "left" else slice(0, m)
        assert (seen["attention_mask"][b, sl] == 1).all() and int(seen["attention_mask"][b].sum()) == m
        assert torch.equal(seen["inputs_embeds"][b, sl], alone["inputs_embeds"][0])
        assert torch.equal(seen["position_ids"][:, b, sl], alone["position_ids"][:, 0])
        if "visual_pos_masks" in alone and alone["visual_pos_masks"] is not None:
            assert torch.equal(seen["visual_pos_masks"][b, sl], alone["visual_pos_masks"][0])
        assert torch.allclose(out.logits[b, sl].float(), one.logits[0].float(), atol=atol, rtol=0)
    OM.set_features(model, merged)


@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_batched_rows_equal_rows_alone(family, side, oracle_pass, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    model = OM.thinker(family)
    merged, rows = _batch(family, side, True)
    OM.set_features(model, merged)
    model.forward = types.MethodType(_hook(family), model)
    calls = _record(model)
    labels = merged["ids"].clone()
    out = model(**merged["kw"], labels=labels)
    keep = model._vidcom2_last.keep_token_indices
    cut = torch.where(keep >= 0, labels.gather(1, keep.clamp(min=0)), torch.full_like(keep, -100))
    assert torch.equal(out.loss, model.loss_function(logits=out.logits, labels=cut, vocab_size=S.VOCAB))
    _check_rows(model, merged, rows, side, calls, out)


@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_batched_generate_equals_rows_alone(family, oracle_pass, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    model = OM.thinker(family)
    merged, rows = _batch(family, "left", True)
    merged_kw = merged["kw"]
    OM.set_features(model, merged)
    model.forward = types.MethodType(_hook(family), model)
    gen = dict(max_new_tokens=3, do_sample=False, eos_token_id=None, pad_token_id=0, output_logits=True,
               return_dict_in_generate=True)
    out = model.generate(**merged_kw, **gen)
    assert model._vidcom2_last.pruned and model._vidcom2_last.keep_token_indices.shape[0] == len(rows)
    _margins_ok(out.logits)
    L = merged["ids"].shape[1]
    for b, r in enumerate(rows):
        OM.set_features(model, r)
        one = model.generate(**r["kw"], **gen)
        for step, (lb, l1) in enumerate(zip(out.logits, one.logits)):
            assert torch.allclose(lb[b], l1[0], atol=1e-4, rtol=0), step
        assert out.sequences[b, L:].tolist() == one.sequences[0, r["ids"].shape[1]:].tolist()


def _bit_identical(model, family, call):
    """`call(model)` with the hook bound == with the thinker's own forward."""
    model.rope_deltas = None
    want = call(model)
    model.forward = types.MethodType(_hook(family), model)
    model.rope_deltas = None
    got = call(model)
    del model.forward
    assert torch.equal(got.logits, want.logits)
    return got


@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_gating_runs_the_thinker_untouched(family, oracle_pass, monkeypatch):
    model = OM.thinker(family)
    p = _prompt(family, "two_videos", True)
    OM.set_features(model, p)
    # knob unset
    monkeypatch.delenv("COMPRESSOR")
    _bit_identical(model, family, lambda m: m(**p["kw"]))
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    # no video
    kw = {k: v for k, v in p["kw"].items() if k not in ("pixel_values_videos", "video_grid_thw")}
    _bit_identical(model, family, lambda m: m(**kw, labels=p["ids"]))
    # a cache that is not empty (the video prompt follows a short text turn)
    pre = model(input_ids=p["ids"][:, :3], attention_mask=torch.ones(1, 3, dtype=torch.int64), use_cache=True)
    deltas = model.rope_deltas
    step = dict(p["kw"], attention_mask=torch.ones(1, 3 + p["ids"].shape[1], dtype=torch.int64))

    def decode(m):
        m.rope_deltas = deltas
        return m(**step, past_key_values=copy.deepcopy(pre.past_key_values))
    _bit_identical(model, family, decode)
    # B > 1 without the batched knob
    merged, _ = _batch(family, "left", True)
    OM.set_features(model, merged)
    _bit_identical(model, family, lambda m: m(**merged["kw"]))


def _router_by_hand(model, dec_kw, labels):
    """aux_loss and loss of the thinker over the decoder inputs `dec_kw` (the kept tokens): its own
    `load_balancing_loss_func` with the mask of those tokens, its own loss function."""
    import sys
    kw = {k: v for k, v in dec_kw.items() if k != "output_router_logits"}
    dec = model.model(**kw, output_router_logits=True)
    aux = sys.modules[type(model).__module__].load_balancing_loss_func(
        dec.router_logits, model.num_experts, model.num_experts_per_tok, kw["attention_mask"])
    logits = model.lm_head(dec.last_hidden_state)
    loss = model.loss_function(logits=logits, labels=labels, vocab_size=S.VOCAB) + model.router_aux_loss_coef * aux
    return aux, loss


@pytest.mark.parametrize("how", ["argument", "config_default"])
@torch.no_grad()
def test_router_loss_over_kept_tokens(how, oracle_pass):
    """Qwen3-Omni with the router load-balancing term: a pruned prefill weighs the router logits of the kept tokens
    with their own (pruned) mask."""
    model = OM.thinker("qwen3_omni")
    p = _prompt("qwen3_omni", "image_and_two_videos", True)
    OM.set_features(model, p)
    model.forward = types.MethodType(_hook("qwen3_omni"), model)
    calls = _record(model)
    extra = {}
    if how == "argument":
        extra["output_router_logits"] = True
    else:
        model.config.text_config.output_router_logits = True
    labels = p["ids"].clone()
    out = model(**p["kw"], labels=labels, **extra)
    _, keep = _keep_by_hand(p)
    assert model._vidcom2_last.pruned and torch.equal(model._vidcom2_last.keep_token_indices, keep)
    _check_decoder_inputs("qwen3_omni", model, p, calls[-1], keep)
    pos, _ = _positions(model, p)
    vpm, deep = _deep_by_hand(p, keep)
    by_hand = dict(inputs_embeds=_embeds(model, p)[:, keep], position_ids=pos[..., keep],
                   attention_mask=p["kw"]["attention_mask"][:, keep], visual_pos_masks=vpm,
                   deepstack_visual_embeds=deep)
    aux, loss = _router_by_hand(model, by_hand, labels[:, keep])
    assert torch.allclose(out.aux_loss, aux, atol=1e-6, rtol=0)
    assert torch.allclose(out.loss, loss, atol=1e-6, rtol=0)
    # without labels: the router term alone, as the thinker reports it
    out = model(**p["kw"], **extra)
    assert out.loss is None and torch.allclose(out.aux_loss, aux, atol=1e-6, rtol=0)


@pytest.mark.parametrize("side", ["left", "right"])
@torch.no_grad()
def test_batched_router_loss_over_kept_tokens(side, oracle_pass, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    model = OM.thinker("qwen3_omni")
    merged, rows = _batch("qwen3_omni", side, True)
    OM.set_features(model, merged)
    model.forward = types.MethodType(_hook("qwen3_omni"), model)
    calls = _record(model)
    labels = merged["ids"].clone()
    out = model(**merged["kw"], labels=labels, output_router_logits=True)
    seen = calls[-1]
    keep = model._vidcom2_last.keep_token_indices
    assert model._vidcom2_last.pruned and seen["attention_mask"].shape == keep.shape
    cut = torch.where(keep >= 0, labels.gather(1, keep.clamp(min=0)), torch.full_like(keep, -100))
    aux, loss = _router_by_hand(model, seen, cut)
    assert torch.allclose(out.aux_loss, aux, atol=1e-6, rtol=0)
    assert torch.allclose(out.loss, loss, atol=1e-6, rtol=0)
    _check_rows(model, merged, rows, side, calls, out)


@torch.no_grad()
def test_router_loss_untouched_when_not_pruning(oracle_pass, monkeypatch):
    """Gated off (knob unset, B > 1 without the batched knob), the thinker's own router term is bit-identical."""
    model = OM.thinker("qwen3_omni")
    p = _prompt("qwen3_omni", "two_videos", True)
    OM.set_features(model, p)
    monkeypatch.delenv("COMPRESSOR")
    got = _bit_identical(model, "qwen3_omni", lambda m: m(**p["kw"], labels=p["ids"], output_router_logits=True))
    assert got.aux_loss is not None
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    merged, _ = _batch("qwen3_omni", "left", True)
    OM.set_features(model, merged)
    model.rope_deltas = None
    want = model(**merged["kw"], labels=merged["ids"], output_router_logits=True)
    model.forward = types.MethodType(_hook("qwen3_omni"), model)
    model.rope_deltas = None
    got = model(**merged["kw"], labels=merged["ids"], output_router_logits=True)
    assert torch.equal(got.aux_loss, want.aux_loss) and torch.equal(got.loss, want.loss)


class _Stop(Exception):
    pass


@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_audio_output_runs_the_thinker_unpruned_with_one_warning(family, oracle_pass):
    from vidcom2_amd.models import install
    model = _outer(family, talker=True)
    th = model.thinker
    p = _prompt(family, "two_videos", True)
    OM.set_features(th, p)
    want = th(**p["kw"]).logits
    seen = []

    def thinker_generate(input_ids=None, **kw):          # the thinker's prefill, then stop before the talker
        seen.append(th(input_ids=input_ids, **{k: v for k, v in kw.items() if k in p["kw"]}))
        raise _Stop

    th.__dict__["generate"] = thinker_generate
    assert install(model)
    asks = [dict(return_audio=True), {}] + ([dict(generation_mode="audio")] if family == "qwen2_5_omni" else [])
    for ask in asks:                                     # explicit, and the has_talker default
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            with pytest.raises(_Stop):
                model.generate(**{k: v for k, v in p["kw"].items() if k != "use_audio_in_video"},
                               use_audio_in_video=True, **ask)
        assert [w.category for w in rec if issubclass(w.category, RuntimeWarning)] == [RuntimeWarning]
        assert torch.equal(seen[-1].logits, want)
        assert not th.__dict__.get("_vidcom2_audio_out", False)
    # text-only generation through the outer model prunes
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        with pytest.raises(_Stop):
            model.generate(**{k: v for k, v in p["kw"].items() if k != "use_audio_in_video"}, use_audio_in_video=True,
                           **({"return_audio": False} if family == "qwen3_omni" else {"generation_mode": "text"}))
    assert not [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert seen[-1].logits.shape[1] < want.shape[1] and th._vidcom2_last.pruned


# ------------------------------------------------------------------------------------------
# GPU: keep indices from the device pass, prompt cut by the fused kernels
# ------------------------------------------------------------------------------------------
DTS = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def _device_keep(feat, grid, merge, base):
    from vidcom2_amd import compress
    t, h, w = (int(v) for v in grid.tolist())
    return compress(feat, (h * w) // (merge ** 2), base, "linear", gather=False).global_idx


def _no_fallback(monkeypatch):
    """Count the fused operations the hook calls (`vidcom2_amd.fused`: B = 1 `keep_positions` + `gather_scatter`,
    B > 1 `keep_positions_batched` + `repad_rows`) and make the torch-indexing layout of B > 1 fail if called."""
    import collections
    import vidcom2_amd.fused as F
    import vidcom2_amd.models._prefill_prune as P

    def boom(*a, **k):
        raise AssertionError("torch fallback used on the device")
    monkeypatch.setattr(P, "_batched_layout", boom)
    counts = collections.Counter()
    for name in ("keep_positions", "gather_scatter", "keep_positions_batched", "repad_rows"):
        def counted(*a, _real=getattr(F, name), _name=name, **k):
            counts[_name] += 1
            return _real(*a, **k)
        monkeypatch.setattr(F, name, counted)
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("audio_in_video", [False, True], ids=["separate_audio", "audio_in_video"])
@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_hooked_decoder_inputs_gpu(family, audio_in_video, dt, monkeypatch):
    fused = _no_fallback(monkeypatch)
    dtype = DTS[dt]
    model = OM.thinker(family, dtype, "cuda")
    p = _prompt(family, "image_and_two_videos", audio_in_video, dtype=dtype)
    OM.set_features(model, p)
    model.forward = types.MethodType(_hook(family), model)
    calls = _record(model)
    kw = OM.to_device(p["kw"], "cuda")
    model(**kw, labels=kw["input_ids"].clone())
    # one keep list, one gather of the prompt rows (+ one of the deep-stack layers)
    assert fused == {"keep_positions": 1, "gather_scatter": 2 if family == "qwen3_omni" else 1}
    kept, keep = _keep_by_hand(p, _device_keep_on_cuda)
    st = model._vidcom2_last
    assert st.pruned and torch.equal(st.keep_token_indices.cpu(), keep)
    if dtype != torch.float32:
        assert torch.equal(kept, _keep_by_hand(p)[0])              # half precision: the oracle's keep list
    _check_decoder_inputs(family, model, {**p, "kw": kw}, calls[-1], keep)


def _device_keep_on_cuda(feat, grid, merge, base):
    return _device_keep(feat.cuda(), grid, merge, base)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("side", ["left", "right"])
@pytest.mark.parametrize("family", FAMILIES)
@torch.no_grad()
def test_batched_rows_gpu_take_the_fused_path(family, side, dt, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    dtype = DTS[dt]
    model = OM.thinker(family, dtype, "cuda")
    merged, rows = _batch(family, side, True, dtype)
    OM.set_features(model, merged)
    model.forward = types.MethodType(_hook(family), model)
    calls = _record(model)
    fused = _no_fallback(monkeypatch)
    out = model(**OM.to_device(merged["kw"], "cuda"))
    assert fused == dict({"keep_positions_batched": 1, "repad_rows": 1},
                         **({"gather_scatter": 1} if family == "qwen3_omni" else {}))
    _check_rows(model, merged, rows, side, calls, out, atol=1e-4 if dtype == torch.float32 else 3e-2)

"""transformers' LLaVA-OneVision / LLaVA-NeXT-Video hooks (`vidcom2_amd.models.llava_hf`) through tiny random-weight
models of the installed transformers (`_llava_hf_models.py`): real towers, real pooling, real decoder stacks, on CPU,
with the device pass replaced by the oracle (as in test_hooks_real_decoder.py).

The yardstick is the UNHOOKED model run on the prompt pruned by hand: `inputs_embeds[:, keep]`, `attention_mask[:, keep]`
and no positions (the reference prunes LLaVA prompts before positions exist), where `keep` is every non-video position,
the oracle's kept video tokens and (OneVision) the newline row.  The `-m gpu` part is test_llava_hf_hooks_gpu.py.
"""
import copy
import inspect

import pytest
import torch

import _llava_hf_models as L
import _stub_models as S
import oracle as O

FRAMES = 8
GEN = dict(max_new_tokens=5, do_sample=False, eos_token_id=None, pad_token_id=0, output_logits=True,
           return_dict_in_generate=True)


def oracle_keep(x, n, base, stats_ws=None):
    x = x.detach()
    return O.compress_indices(x.contiguous().cpu(), n, base)["global_idx"].to(x.device)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    O.set_mode("torch")
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", "0.5")
    monkeypatch.delenv("VC2_BATCHED_PREFILL", raising=False)
    monkeypatch.delenv("VC2_FUSED_POOL", raising=False)
    import vidcom2_amd.models._prefill_prune as P
    import vidcom2_amd.models.llava_hf as H
    monkeypatch.setattr(P, "_WARNED", set())
    monkeypatch.setattr(H, "_keep_indices", oracle_keep)
    monkeypatch.setattr(H, "_keep_indices_many", lambda xs, n, base: [oracle_keep(x, n, base) for x in xs])


def _hooks(family):
    import vidcom2_amd.models.llava_hf as H
    if family == "onevision":
        return H.LlavaOnevisionModel_forward, H.LlavaOnevisionForConditionalGeneration_forward
    return H.LlavaNextVideoModel_forward, H.LlavaNextVideoForConditionalGeneration_forward


def hooked_and_plain(family, outer=True):
    """Two models of the same weights: one with the hook installed, one untouched."""
    from vidcom2_amd.models import install
    hooked, plain = L.model(family, outer=outer), L.model(family, outer=outer)
    assert install(hooked)
    return hooked, plain


def dense_embeds(plain_inner, kw):
    """The prompt embeddings the unhooked model hands its decoder (every modality scattered in)."""
    calls = L.record(plain_inner)
    out = plain_inner(**kw)
    return calls[-1]["inputs_embeds"], out


def keep_by_hand(family, ids_row, emb_row, ratio, frames=FRAMES):
    """(video features, kept video ordinals, kept positions) of one row: the oracle's kept tokens of the row's video, its
    newline row (OneVision), every non-video position."""
    n = L.TPF[family]
    vm = ids_row == S.VIDEO_ID
    vpos = vm.nonzero().squeeze(-1)
    feats = emb_row[vpos]
    kept = O.compress_indices(feats[:frames * n].contiguous(), n, ratio)["global_idx"]
    assert 0 < kept.numel() < frames * n            # a strict, non-empty subset: the comparison below means something
    if L.NEWLINE[family]:
        kept = torch.cat((kept, torch.tensor([frames * n])))
    flags = ~vm
    flags[vpos[kept]] = True
    return feats, kept, flags.nonzero().squeeze(-1)


def _margins_ok(logits):
    for step in logits:
        top = step.float().topk(2, dim=-1).values
        assert ((top[:, 0] - top[:, 1]) > 1e-3).all(), "top-2 logits too close for token equality to mean anything"


# ------------------------------------------------------------------------------------------
# 1. install()
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
def test_install_binds_on_outer_model_and_bare_model(family):
    from vidcom2_amd.models import install
    inner_hook, outer_hook = _hooks(family)
    model = L.model(family)
    assert install(model) is True
    assert model.model.forward.__func__ is inner_hook and model.model.__dict__["forward"].__self__ is model.model
    assert model.__dict__["forward"].__func__ is outer_hook
    bare = L.model(family, outer=False)
    assert install(bare) is True
    assert bare.forward.__func__ is inner_hook
    Outer, Inner = L.classes(family)
    # the hooks show the parameters of the forwards they wrap (generate validates its keyword arguments against them)
    assert list(inspect.signature(bare.forward).parameters) == list(inspect.signature(Inner.forward).parameters)[1:]
    assert list(inspect.signature(model.forward).parameters) == list(inspect.signature(Outer.forward).parameters)[1:]


def test_install_needs_the_knob(monkeypatch):
    from vidcom2_amd.models import install
    monkeypatch.delenv("COMPRESSOR")
    model = L.model("onevision")
    assert install(model) is False and "forward" not in model.model.__dict__ and "forward" not in model.__dict__


# ------------------------------------------------------------------------------------------
# 2. + 3. the hooked forward == the unhooked model on the prompt pruned by hand
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("positions", ["given", "absent"])
@pytest.mark.parametrize("ratio", [0.5, 0.25])
@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_hook_equals_hand_pruned_run(family, ratio, positions, monkeypatch):
    monkeypatch.setenv("R_RATIO", str(ratio))
    hooked, plain = hooked_and_plain(family, outer=False)
    kw = L.prompt(family, FRAMES, seed=3, n_image=L.image_tokens(plain))
    ids, mask = kw["input_ids"], kw["attention_mask"]
    emb, dense = dense_embeds(plain, kw)
    calls = L.record(hooked)
    extra = dict(position_ids=torch.arange(ids.shape[1])[None]) if positions == "given" else {}
    out = hooked(**kw, **extra).last_hidden_state
    st = hooked._vidcom2_last
    feats, kept, keep = keep_by_hand(family, ids[0], emb[0], ratio)
    assert st.pruned and torch.equal(st.video_embeds, feats)
    assert torch.equal(st.kept_video, kept) and torch.equal(st.keep_token_indices, keep)
    assert st.lengths.tolist() == [keep.numel()]
    assert (ids[0, keep] != S.VIDEO_ID).sum() == (ids[0] != S.VIDEO_ID).sum()        # text and image: all kept
    assert int((ids[0] == S.IMAGE_ID).sum()) > 0
    Sp = keep.numel()
    assert out.shape[1] == Sp < ids.shape[1]
    seen = calls[-1]
    assert torch.equal(seen["inputs_embeds"], emb[:, keep]) and torch.equal(seen["attention_mask"], mask[:, keep])
    if positions == "given":
        assert torch.equal(seen["position_ids"], torch.arange(Sp)[None])             # numbered 0 .. S'-1
    else:
        assert seen["position_ids"] is None
    manual = plain(inputs_embeds=emb[:, keep], attention_mask=mask[:, keep]).last_hidden_state
    assert torch.allclose(out, manual, atol=1e-6)
    # and pruning really changes what the decoder computes
    assert not torch.allclose(out, dense.last_hidden_state[:, keep], atol=1e-3)


@pytest.mark.parametrize("ratio", [0.5, 0.25])
@torch.no_grad()
def test_onevision_kept_rows_are_the_llava_ov_rows_then_the_newline(ratio, monkeypatch):
    """At n = 196 the kept video rows are those `vidcom2_compression(x, "llava_ov", ratio)` returns -- x[the oracle's
    indices] -- followed by the newline row (the reference hook's one_token branch)."""
    monkeypatch.setenv("R_RATIO", str(ratio))
    hooked, plain = hooked_and_plain("onevision", outer=False)
    kw = L.prompt("onevision", FRAMES, seed=4)
    emb, _ = dense_embeds(plain, kw)
    calls = L.record(hooked)
    hooked(**kw)
    st = hooked._vidcom2_last
    x = st.video_embeds[:FRAMES * 196]
    idx = O.compress_indices(x.contiguous(), 196, ratio)["global_idx"]
    assert 0 < idx.numel() < FRAMES * 196
    assert torch.equal(st.kept_video, torch.cat((idx, torch.tensor([FRAMES * 196]))))
    ids = kw["input_ids"][0]
    rows = calls[-1]["inputs_embeds"][0, ids[st.keep_token_indices] == S.VIDEO_ID]
    assert torch.equal(rows, torch.cat((x[idx], plain.image_newline[None])))
    assert torch.equal(st.video_embeds[-1], plain.image_newline)


# ------------------------------------------------------------------------------------------
# 4. generate(): the decode steps behind a pruned prefill
# ------------------------------------------------------------------------------------------
def _generate_by_hand(plain, emb, mask, keeps):
    """The unhooked model's generate on the hand-pruned prompts, left-padded to the longest one."""
    Sp = max(k.numel() for k in keeps)
    e = emb.new_zeros(len(keeps), Sp, emb.shape[-1])
    m = mask.new_zeros(len(keeps), Sp)
    for b, k in enumerate(keeps):
        e[b, Sp - k.numel():], m[b, Sp - k.numel():] = emb[b, k], mask[b, k]
    return plain.generate(inputs_embeds=e, attention_mask=m, **GEN)


@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_generate_equals_generate_on_the_hand_pruned_prompt(family):
    hooked, plain = hooked_and_plain(family)
    kw = L.prompt(family, FRAMES, seed=5, n_image=L.image_tokens(plain.model))
    emb, _ = dense_embeds(plain.model, kw)
    calls = L.record(hooked.model)
    gen = hooked.generate(**kw, **GEN)
    _, _, keep = keep_by_hand(family, kw["input_ids"][0], emb[0], 0.5)
    S0, Sp = kw["input_ids"].shape[1], keep.numel()
    assert hooked.model._vidcom2_last.pruned and Sp < S0
    want = _generate_by_hand(plain, emb, kw["attention_mask"], [keep])
    _margins_ok(want.logits)
    assert gen.sequences[0, S0:].tolist() == want.sequences[0].tolist() and len(want.sequences[0]) == 5
    for a, b in zip(gen.logits, want.logits):
        assert torch.allclose(a, b, atol=1e-5, rtol=0)
    # what the decoder saw: prefill 0 .. S'-1, then step t at position S' + t - 1 under a mask of S' + t columns
    assert len(calls) == 5 and torch.equal(calls[0]["position_ids"], torch.arange(Sp)[None])
    for t in range(1, 5):
        assert calls[t]["position_ids"].tolist() == [[Sp + t - 1]]
        assert tuple(calls[t]["attention_mask"].shape) == (1, Sp + t) and bool(calls[t]["attention_mask"].all())


@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_batched_generate_equals_hand_pruned_batch_and_rows_alone(family, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    hooked, plain = hooked_and_plain(family)
    rows = [L.prompt(family, FRAMES, seed=5, prefix=6, suffix=5, n_image=L.image_tokens(plain.model)),
            L.prompt(family, FRAMES, seed=15, prefix=11, suffix=3)]
    kw = L.batch(rows, "left")
    ids, mask = kw["input_ids"], kw["attention_mask"]
    assert (mask[1] == 0).any() and mask[0].all()                       # different prompt lengths, left-padded
    emb, _ = dense_embeds(plain.model, kw)
    keeps = [keep_by_hand(family, ids[b], emb[b], 0.5)[2] for b in range(2)]
    calls = L.record(hooked.model)
    gen = hooked.generate(**kw, **GEN)
    st = hooked.model._vidcom2_last
    Sp = max(k.numel() for k in keeps)
    assert st.pruned and tuple(st.keep_token_indices.shape) == (2, Sp) and Sp < ids.shape[1]
    assert st.lengths.tolist() == [k.numel() for k in keeps]
    want = _generate_by_hand(plain, emb, mask, keeps)
    _margins_ok(want.logits)
    assert gen.sequences[:, ids.shape[1]:].tolist() == want.sequences.tolist()
    # the decoder inputs of every step are those of the hand-pruned batch
    plain_calls = L.record(plain.model)
    _generate_by_hand(plain, emb, mask, keeps)
    assert len(calls) == len(plain_calls) == 5
    for got, ref in zip(calls, plain_calls):
        assert torch.equal(got["position_ids"], ref["position_ids"])
        assert torch.equal(got["attention_mask"], ref["attention_mask"])
    assert torch.equal(calls[0]["inputs_embeds"], plain_calls[0]["inputs_embeds"])
    # every row equals its own B = 1 run
    for b, r in enumerate(rows):
        one = hooked.generate(**r, **GEN)
        _margins_ok(one.logits)
        assert gen.sequences[b, ids.shape[1]:].tolist() == one.sequences[0, r["input_ids"].shape[1]:].tolist()
        for lb, l1 in zip(gen.logits, one.logits):
            assert torch.allclose(lb[b], l1[0], atol=1e-4, rtol=0)


# ------------------------------------------------------------------------------------------
# 5. inactive paths: bit-identical to the unhooked model
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_gating_runs_the_model_untouched(family, monkeypatch):
    hooked, plain = hooked_and_plain(family)
    n_image = L.image_tokens(plain.model)
    video = L.prompt(family, FRAMES, seed=6, n_image=n_image)

    def same(kw, **more):
        hooked.model.__dict__.pop("_vidcom2_last", None)
        got, want = hooked(**kw, **copy.deepcopy(more)), plain(**kw, **copy.deepcopy(more))     # (a cache grows in place)
        assert torch.equal(got.logits, want.logits)
        assert "_vidcom2_last" not in hooked.model.__dict__ or not hooked.model._vidcom2_last.pruned
        return got

    # knob unset
    monkeypatch.delenv("COMPRESSOR")
    same(video)
    got = same(video, labels=video["input_ids"])
    assert torch.equal(got.loss, plain(**video, labels=video["input_ids"]).loss)
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    # an image-only prompt
    image = L.prompt(family, FRAMES, seed=6, n_image=n_image, video=False)
    got = same(image, labels=image["input_ids"])
    assert torch.equal(got.loss, plain(**image, labels=image["input_ids"]).loss)
    # B = 2 without VC2_BATCHED_PREFILL
    same(L.batch([video, L.prompt(family, FRAMES, seed=16, prefix=9)], "left"))
    # a decode step called directly with a cache that is not empty (the video prompt follows a short text turn)
    pre = plain(input_ids=video["input_ids"][:, :3], use_cache=True)
    step = dict(video, input_ids=video["input_ids"][:, 3:])
    same(step, past_key_values=pre.past_key_values)


# ------------------------------------------------------------------------------------------
# 6. labels
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
def test_labels_give_the_loss_of_the_hand_pruned_run(family):
    hooked, plain = hooked_and_plain(family)
    kw = L.prompt(family, FRAMES, seed=7, n_image=L.image_tokens(plain.model))
    ids, mask = kw["input_ids"], kw["attention_mask"]
    labels = ids.clone()
    labels[:, :4] = -100
    with torch.no_grad():
        emb, _ = dense_embeds(plain.model, kw)
        _, _, keep = keep_by_hand(family, ids[0], emb[0], 0.5)
        out = hooked(**kw, labels=labels)
        logits = plain(inputs_embeds=emb[:, keep], attention_mask=mask[:, keep]).logits
        want = plain.loss_function(logits=logits, labels=labels[:, keep], vocab_size=S.VOCAB)
        assert out.logits.shape[1] == keep.numel() < ids.shape[1]
        assert torch.allclose(out.logits, logits, atol=1e-5, rtol=0)
        assert torch.allclose(out.loss, want)
        assert torch.equal(out.loss, plain.loss_function(logits=out.logits, labels=labels[:, keep], vocab_size=S.VOCAB))
        # return_dict=False and logits_to_keep keep working
        tup = hooked(**kw, labels=labels, return_dict=False)
        assert isinstance(tup, tuple) and torch.equal(tup[0], out.loss) and torch.equal(tup[1], out.logits)
        last = hooked(**kw, logits_to_keep=1)
        assert last.loss is None and tuple(last.logits.shape) == (1, 1, S.VOCAB)
        assert torch.allclose(last.logits, out.logits[:, -1:], atol=1e-6, rtol=0)     # (another GEMM shape: not bits)
    # gradients reach the newline, the projector and the embedding table
    hooked.zero_grad()
    hooked(**kw, labels=labels).loss.backward()
    inner = hooked.model
    for name, p in (("image_newline", inner.image_newline), ("projector", inner.multi_modal_projector.linear_1.weight),
                    ("embedding", inner.get_input_embeddings().weight)):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name


@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_batched_labels_carry_minus_100_in_pad_slots(family, monkeypatch):
    monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    hooked, plain = hooked_and_plain(family)
    kw = L.batch([L.prompt(family, FRAMES, seed=5, prefix=6), L.prompt(family, FRAMES, seed=15, prefix=11, suffix=3)],
                 "right")
    labels = kw["input_ids"].clone()
    out = hooked(**kw, labels=labels)
    keep = hooked.model._vidcom2_last.keep_token_indices
    assert (keep < 0).any()
    cut = torch.where(keep >= 0, labels.gather(1, keep.clamp(min=0)), torch.full_like(keep, -100))
    assert torch.equal(out.loss, plain.loss_function(logits=out.logits, labels=cut, vocab_size=S.VOCAB))


@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_two_videos_in_one_prompt_are_scored_one_by_one(family):
    """B = 1 with two entries in `pixel_values_videos`: each video scored alone, each newline kept."""
    hooked, plain = hooked_and_plain(family, outer=False)
    a, b = L.prompt(family, FRAMES, seed=8, prefix=5, suffix=3), L.prompt(family, FRAMES, seed=18, prefix=2, suffix=6)
    ids = torch.cat((a["input_ids"], b["input_ids"]), 1)
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids),
              pixel_values_videos=torch.cat((a["pixel_values_videos"], b["pixel_values_videos"])))
    emb, _ = dense_embeds(plain, kw)
    out = hooked(**kw).last_hidden_state
    st = hooked._vidcom2_last
    n, extra = L.TPF[family], 1 if L.NEWLINE[family] else 0
    per = FRAMES * n + extra
    vpos = (ids[0] == S.VIDEO_ID).nonzero().squeeze(-1)
    assert vpos.numel() == 2 * per
    kept = []
    for c in range(2):
        idx = O.compress_indices(emb[0, vpos[c * per: c * per + FRAMES * n]].contiguous(), n, 0.5)["global_idx"]
        assert 0 < idx.numel() < FRAMES * n
        kept.append(idx + c * per)
        if extra:
            kept.append(torch.tensor([c * per + FRAMES * n]))
    kept = torch.cat(kept)
    flags = ids[0] != S.VIDEO_ID
    flags[vpos[kept]] = True
    keep = flags.nonzero().squeeze(-1)
    assert st.pruned and torch.equal(st.kept_video, kept) and torch.equal(st.keep_token_indices, keep)
    manual = plain(inputs_embeds=emb[:, keep], attention_mask=kw["attention_mask"][:, keep]).last_hidden_state
    assert torch.allclose(out, manual, atol=1e-6)

"""The `-m gpu` part of test_llava_hf_hooks.py: the transformers LLaVA hooks on the device, in bf16 and fp16 -- keep
indices from the device pass, the prompt cut by the fused kernels (`keep_positions` + `gather_scatter`, B > 1:
`compress_batch` lanes + `keep_positions_batched` + `repad_rows`), the optional fused pooling (`VC2_FUSED_POOL=on`).
Video features are synthetic and injected (`_llava_hf_models.set_video_features`) except where the pooling itself is
under test."""
import collections
import ctypes
import logging

import pytest
import torch

import _llava_hf_models as L
import _stub_models as S
import oracle as O
from vidcom2_amd.models._prefill_prune import _batched_layout, _gather_slots      # (the definition, before any patching)

pytestmark = pytest.mark.gpu

FRAMES = 8
R = 0.5
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}
GEN = dict(max_new_tokens=5, do_sample=False, eos_token_id=None, pad_token_id=0, output_logits=True,
           return_dict_in_generate=True)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    O.set_mode("torch")
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", str(R))
    monkeypatch.delenv("VC2_BATCHED_PREFILL", raising=False)
    monkeypatch.delenv("VC2_FUSED_POOL", raising=False)
    import vidcom2_amd.models._prefill_prune as P
    monkeypatch.setattr(P, "_WARNED", set())
    yield
    from vidcom2_amd._ffi import check, lib
    out = (ctypes.c_int32 * 8)()
    check(lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    assert list(out) == [0] * 8, list(out)                  # no bounded loop of the engine expired


def _no_fallback(monkeypatch):
    """Count the fused operations the hook calls and make the torch-indexing layout of B > 1 fail if called."""
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


def _rows(family, B, dtype, D=L.D):
    """B prompts of different lengths with injected video features; (rows, feats per row [F, n, D])."""
    specs = [dict(prefix=6, suffix=5), dict(prefix=11, suffix=3), dict(prefix=4, suffix=9)][:B]
    rows = [L.prompt(family, FRAMES, seed=5 + 10 * i, pixels=False, dtype=dtype, **s) for i, s in enumerate(specs)]
    feats = [S.video_feats(FRAMES, L.TPF[family], D, dtype, 21 + i) for i in range(B)]
    return rows, feats


def _by_hand(family, inner, kw, feats):
    """Unpruned prompt embeddings with the features scattered in (CPU), per row kept video ordinals (oracle) and kept
    positions."""
    ids = kw["input_ids"]
    n = L.TPF[family]
    table = inner.get_input_embeddings().weight.detach().cpu()
    emb = table[ids]
    kept, keeps = [], []
    for b, f in enumerate(feats):
        x = f.reshape(-1, f.shape[-1])
        full = torch.cat((x, inner.image_newline.detach().cpu()[None])) if L.NEWLINE[family] else x
        vm = ids[b] == S.VIDEO_ID
        emb[b, vm] = full
        idx = O.compress_indices(x.contiguous(), n, R)["global_idx"]
        assert 0 < idx.numel() < FRAMES * n
        if L.NEWLINE[family]:
            idx = torch.cat((idx, torch.tensor([FRAMES * n])))
        flags = ~vm
        flags[vm.nonzero().squeeze(-1)[idx]] = True
        kept.append(idx + b * full.shape[0])
        keeps.append(flags.nonzero().squeeze(-1))
    return emb, torch.cat(kept), keeps


def _generate_positions(mask):
    """The positions generate derives from a mask."""
    return (mask.cumsum(-1) - 1).masked_fill(mask == 0, 0)


def _check_decoder_inputs(family, inner, kw, feats, seen, st, B):
    emb, kept, keeps = _by_hand(family, inner, kw, feats)
    ids, mask = kw["input_ids"], kw["attention_mask"]
    assert st.pruned and torch.equal(st.kept_video.cpu(), kept)
    if B == 1:
        keep = keeps[0]
        assert torch.equal(st.keep_token_indices.cpu(), keep)
        want_emb, want_mask = emb[:, keep], mask[:, keep]
    else:
        lay = _batched_layout(ids == S.VIDEO_ID, kept, True, mask, _generate_positions(mask)[None], True)
        assert torch.equal(st.keep_token_indices.cpu(), lay.keep) and lay.lengths.tolist() == [k.numel() for k in keeps]
        for b, k in enumerate(keeps):                                   # the layout: every row's own list, left-padded
            assert torch.equal(lay.keep[b, lay.S - k.numel():], k) and (lay.keep[b, :lay.S - k.numel()] == -1).all()
        want_emb, want_mask = _gather_slots(emb, lay.keep, 0), lay.mask
        assert torch.equal(seen["position_ids"].cpu(), lay.pos[0])
    Sp = want_mask.shape[1]
    assert Sp < ids.shape[1]
    assert torch.equal(seen["inputs_embeds"].cpu(), want_emb)
    assert torch.equal(seen["attention_mask"].cpu(), want_mask)
    # ... which is what generate hands the decoder for the hand-pruned prompt
    assert torch.equal(seen["position_ids"].cpu(), _generate_positions(want_mask))
    assert torch.equal(seen["cache_position"].cpu(), torch.arange(Sp))
    assert st.lengths.cpu().tolist() == [k.numel() for k in keeps]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_decoder_inputs_gpu(family, dt, B, monkeypatch):
    from vidcom2_amd.models import install
    if B > 1:
        monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    dtype = DTS[dt]
    inner = L.model(family, dtype, "cuda", outer=False)
    rows, feats = _rows(family, B, dtype)
    kw = L.batch(rows, "left") if B > 1 else rows[0]
    L.set_video_features(inner, family, [f.cuda() for f in feats])
    assert install(inner)
    calls = L.record(inner)
    fused = _no_fallback(monkeypatch)
    dev = L.to_device(kw, "cuda")
    S0 = kw["input_ids"].shape[1]
    inner(**dev, position_ids=_generate_positions(dev["attention_mask"]), cache_position=torch.arange(S0, device="cuda"))
    assert fused == ({"keep_positions": 1, "gather_scatter": 1} if B == 1 else
                     {"keep_positions_batched": 1, "repad_rows": 1})
    _check_decoder_inputs(family, inner, kw, feats, calls[-1], inner._vidcom2_last, B)


@torch.no_grad()
def test_decoder_inputs_gpu_at_onevision_7b_width(monkeypatch):
    """D = 3584 (LLaVA-OneVision-7B's text width), bf16: the decoder stack is a recorder, everything before it is the
    model's own forward."""
    from vidcom2_amd.models import install
    Dw, dtype = 3584, torch.bfloat16
    _, Inner = L.classes("onevision")
    with torch.device("meta"):
        inner = Inner(L.config("onevision", hidden=Dw, layers=1))
    inner.language_model = None
    rec = S.Recorder(S.embed_table(Dw, dtype, 9).cuda())
    inner.language_model = rec
    inner.image_newline = torch.nn.Parameter(S.newline_vec(Dw, dtype, 9).cuda(), requires_grad=False)
    inner.eval()
    rows, feats = _rows("onevision", 1, dtype, Dw)
    L.set_video_features(inner, "onevision", [f.cuda() for f in feats])
    assert install(inner)
    fused = _no_fallback(monkeypatch)
    dev = L.to_device(rows[0], "cuda")
    S0 = rows[0]["input_ids"].shape[1]
    inner(**dev, position_ids=torch.arange(S0, device="cuda")[None], cache_position=torch.arange(S0, device="cuda"))
    assert fused == {"keep_positions": 1, "gather_scatter": 1}
    _check_decoder_inputs("onevision", inner, rows[0], feats, rec.calls[-1], inner._vidcom2_last, 1)


def _generate_by_hand(plain, emb, mask, keeps):
    Sp = max(k.numel() for k in keeps)
    e = emb.new_zeros(len(keeps), Sp, emb.shape[-1])
    m = mask.new_zeros(len(keeps), Sp)
    for b, k in enumerate(keeps):
        e[b, Sp - k.numel():], m[b, Sp - k.numel():] = emb[b, k], mask[b, k]
    return plain.generate(inputs_embeds=e.cuda(), attention_mask=m.cuda(), **GEN)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("family", L.FAMILIES)
@torch.no_grad()
def test_generate_gpu(family, dt, B, monkeypatch):
    """Greedy generate through the hook == the unhooked model's generate on the hand-pruned prompts, five steps; every
    row of a batch == its own B = 1 run."""
    from vidcom2_amd.models import install
    if B > 1:
        monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    dtype = DTS[dt]
    hooked, plain = L.model(family, dtype, "cuda"), L.model(family, dtype, "cuda")
    rows, feats = _rows(family, B, dtype)
    kw = L.batch(rows, "left") if B > 1 else rows[0]
    L.set_video_features(hooked.model, family, [f.cuda() for f in feats])
    assert install(hooked)
    calls = L.record(hooked.model)
    gen = hooked.generate(**L.to_device(kw, "cuda"), **GEN)
    emb, _, keeps = _by_hand(family, plain.model, kw, feats)
    S0 = kw["input_ids"].shape[1]
    assert hooked.model._vidcom2_last.pruned and len(calls) == 5
    plain_calls = L.record(plain.model)
    want = _generate_by_hand(plain, emb, kw["attention_mask"], keeps)
    for got, ref in zip(calls, plain_calls):                           # every step's decoder inputs
        assert torch.equal(got["position_ids"], ref["position_ids"])
        assert torch.equal(got["attention_mask"], ref["attention_mask"])
        assert torch.equal(got["inputs_embeds"], ref["inputs_embeds"])
    assert gen.sequences[:, S0:].tolist() == want.sequences.tolist() and want.sequences.shape[1] == 5
    if B > 1:
        for b, r in enumerate(rows):
            L.set_video_features(hooked.model, family, [feats[b].cuda()])
            one = hooked.generate(**L.to_device(r, "cuda"), **GEN)
            assert gen.sequences[b, S0:].tolist() == one.sequences[0, r["input_ids"].shape[1]:].tolist()


# ------------------------------------------------------------------------------------------
# fused pooling (OneVision, VC2_FUSED_POOL=on)
# ------------------------------------------------------------------------------------------
def _watch_pooling(inner):
    """What `apply_pooling` is while the forward runs, and what it is given."""
    seen = []
    inner.multi_modal_projector.register_forward_hook(
        lambda mod, args, out: seen.append((inner.apply_pooling, out.detach())))
    return seen


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("dt", list(DTS))
@torch.no_grad()
def test_fused_pool_gpu(dt, B, monkeypatch, caplog):
    import vidcom2_amd.models.llava_hf as H
    from vidcom2_amd import compress
    from vidcom2_amd.models import install
    monkeypatch.setenv("VC2_FUSED_POOL", "on")
    monkeypatch.setattr(H, "_POOL_LOGGED", [False])
    if B > 1:
        monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    dtype = DTS[dt]
    _, Inner = L.classes("onevision")
    inner = L.model("onevision", dtype, "cuda", outer=False)
    rows = [L.prompt("onevision", FRAMES, seed=5 + 10 * i, prefix=6 + 5 * i, dtype=dtype) for i in range(B)]
    kw = L.to_device(L.batch(rows, "left") if B > 1 else rows[0], "cuda")
    assert install(inner)
    seen = _watch_pooling(inner)
    handed = []

    def watched(x, n, base, stats_ws=None, _real=H._keep_indices):
        # the statistics are handed over, and for exactly this tensor (compress would otherwise run sweep 1 again)
        handed.append(stats_ws is not None and stats_ws._vc2_stats_for == (x.shape[0] // n, n, x.shape[1], x.dtype,
                                                                          x.data_ptr()))
        return _real(x, n, base, stats_ws)
    monkeypatch.setattr(H, "_keep_indices", watched)
    with caplog.at_level(logging.WARNING, logger=H.__name__):
        inner(**kw)
        inner(**kw)
    assert len([r for r in caplog.records if "VC2_FUSED_POOL" in r.getMessage()]) == 1       # said once
    assert handed == [True] * (2 * B)
    st = inner._vidcom2_last
    shadowed, projected = seen[-1]
    assert getattr(shadowed, "__func__", None) is not Inner.apply_pooling and "apply_pooling" not in inner.__dict__
    # the pooled tensor: the bits of the model's own pooling on a CPU copy
    want = inner.apply_pooling(projected.cpu()).reshape(B, FRAMES * 196, -1)
    per = FRAMES * 196 + 1
    got = st.video_embeds.view(B, per, -1)
    assert torch.equal(got[:, :-1].cpu(), want)
    # the kept set: the pass on that pooled tensor, without the statistics hand-over
    kept = []
    for b in range(B):
        idx = compress(got[b, :-1].contiguous(), 196, R, gather=False).global_idx
        assert 0 < idx.numel() < FRAMES * 196
        kept += [idx + b * per, torch.tensor([b * per + FRAMES * 196], device="cuda")]
    assert st.pruned and torch.equal(st.kept_video, torch.cat(kept))


@torch.no_grad()
def test_pooling_is_the_models_own_without_the_knob(monkeypatch):
    from vidcom2_amd.models import install
    _, Inner = L.classes("onevision")
    inner = L.model("onevision", torch.bfloat16, "cuda", outer=False)
    kw = L.to_device(L.prompt("onevision", FRAMES, seed=5, dtype=torch.bfloat16), "cuda")
    assert install(inner)
    seen = _watch_pooling(inner)
    inner(**kw)
    assert inner._vidcom2_last.pruned
    assert seen[-1][0].__func__ is Inner.apply_pooling and seen[-1][0].__self__ is inner


@pytest.mark.parametrize("ratio", [0.5, 0.25])
@torch.no_grad()
def test_onevision_kept_rows_are_vidcom2_compression_rows_gpu(ratio, monkeypatch):
    """At n = 196 the kept video rows reaching the decoder are `vidcom2_compression(x, "llava_ov", ratio)` followed by
    the newline row, bit for bit."""
    from vidcom2_amd import vidcom2_compression
    from vidcom2_amd.models import install
    monkeypatch.setenv("R_RATIO", str(ratio))
    dtype = torch.bfloat16
    inner = L.model("onevision", dtype, "cuda", outer=False)
    rows, feats = _rows("onevision", 1, dtype)
    L.set_video_features(inner, "onevision", [f.cuda() for f in feats])
    assert install(inner)
    calls = L.record(inner)
    inner(**L.to_device(rows[0], "cuda"))
    st = inner._vidcom2_last
    x = st.video_embeds[:FRAMES * 196]
    want = torch.cat((vidcom2_compression(x.contiguous(), "llava_ov", ratio), inner.image_newline[None]))
    ids = rows[0]["input_ids"][0].cuda()
    got = calls[-1]["inputs_embeds"][0, ids[st.keep_token_indices] == S.VIDEO_ID]
    assert 1 < got.shape[0] < FRAMES * 196 and torch.equal(got, want)


# ------------------------------------------------------------------------------------------
# labels and gradients through the fused gathers
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("family", L.FAMILIES)
def test_labels_loss_backpropagates_like_torch_indexing_gpu(family, B, monkeypatch):
    """fp32, real towers: the loss over the pruned sequence and its gradients on the newline, the projector and the
    embedding table are those of the torch-indexing path (the fused gathers' backward, `vidcom2_amd/autograd.py`)."""
    import vidcom2_amd.models._prefill_prune as P
    from vidcom2_amd.models import install
    if B > 1:
        monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    model = L.model(family, torch.float32, "cuda")
    with torch.no_grad():
        n_image = L.image_tokens(model.model)
    rows = [L.prompt(family, FRAMES, seed=5 + 10 * i, prefix=6 + 5 * i, n_image=n_image if i == 0 else 0)
            for i in range(B)]
    kw = L.to_device(L.batch(rows, "right") if B > 1 else rows[0], "cuda")
    labels = kw["input_ids"].clone()
    assert install(model)
    inner = model.model
    params = dict(newline=inner.image_newline, projector=inner.multi_modal_projector.linear_1.weight,
                  embedding=inner.get_input_embeddings().weight)

    def run():
        model.zero_grad()
        out = model(**kw, labels=labels)
        out.loss.backward()
        st = inner._vidcom2_last
        assert st.pruned and out.logits.shape[1] == st.keep_token_indices.shape[-1] < labels.shape[1]
        return out.loss.detach(), {k: p.grad.clone() for k, p in params.items()}, st.keep_token_indices

    fused = _no_fallback(monkeypatch)
    loss, grads, keep = run()
    assert fused == ({"keep_positions": 1, "gather_scatter": 1} if B == 1 else
                     {"keep_positions_batched": 1, "repad_rows": 1})
    monkeypatch.undo()                                      # (the env of the fixture goes too)
    monkeypatch.setenv("COMPRESSOR", "vidcom2")
    monkeypatch.setenv("R_RATIO", str(R))
    if B > 1:
        monkeypatch.setenv("VC2_BATCHED_PREFILL", "1")
    monkeypatch.setattr(P, "_fusable", lambda *a, **k: False)
    loss_t, grads_t, keep_t = run()
    assert torch.equal(keep, keep_t) and torch.allclose(loss, loss_t, atol=1e-6, rtol=0)
    for k in params:
        assert torch.isfinite(grads[k]).all() and grads[k].abs().sum() > 0, k
        assert torch.allclose(grads[k], grads_t[k], atol=1e-6, rtol=1e-5), k

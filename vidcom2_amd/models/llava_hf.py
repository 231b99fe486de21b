"""transformers' LLaVA-OneVision / LLaVA-NeXT-Video hooks: video-token pruning in the prefill.

    model.model.forward = types.MethodType(LlavaOnevisionModel_forward, model.model)    # or vidcom2_amd.models.install(model)

Provenance: the reference has no hook for the transformers classes (its LLaVA hook patches the LLaVA-NeXT package's
`prepare_inputs_labels_for_multimodal`, `llava.py` here).  The semantics are that hook's `one_token` branch
(token_compressor/vidcom2/models/llava.py:154-168) carried over to `LlavaOnevisionModel` / `LlavaNextVideoModel`, pinned
against the oracle's stage chain and a by-hand pruned run of the unhooked model, not against a golden of a reference hook.

What the hooks do, on top of the shared interceptor (`_prefill_prune.py`, `renumber=True`):

* gating is the Qwen2.5-VL hook's: `COMPRESSOR=vidcom2`, `pixel_values_videos` given, empty KV cache, B = 1 or
  `VC2_BATCHED_PREFILL=1`; otherwise the model's own forward runs untouched;
* every video (one entry of `pixel_values_videos [videos, F, C, H, W]`; one per batch row in the usual call) is scored
  on its own with `R_RATIO`.
  OneVision: the row's features are F*n pooled tokens followed by ONE `image_newline` row; the first F*n go through
  `compress(x, n, ratio, gather=False)` and the newline ordinal F*n is always kept.  LLaVA-NeXT-Video: F*n tokens from
  `vision_resampler` + projector, no newline.  Image placeholders, text and padding are never dropped;
* positions: the reference prunes LLaVA prompts BEFORE positions exist, so the pruned prompt is numbered 0 .. S'-1 and
  decoding continues at S' -- NOT the Qwen hooks' sliced positions.  A `position_ids [B, S]` that generate hands over is
  lowered at every kept position by the number of that row's dropped tokens before it; the decode steps behind a pruned
  prefill get their mask mapped onto the pruned KV cache and their positions lowered by the row's dropped count;
* `labels` (outer `*ForConditionalGeneration.forward`, wrapped by `install()`): gathered with the same keep list (-100
  in the pad slots of a batch), the loss is the model's own `loss_function` over the logits of the pruned sequence;
* `VC2_FUSED_POOL=on` (OneVision, opt-in): `apply_pooling` is shadowed by `fused.pool_stats(x, side, side, "bilinear")`,
  whose statistics workspace lets the pass skip its first sweep.  The fused pooling reproduces torch's CPU bilinear
  bits, which may differ by rounding from the GPU `interpolate` the model ran before `install()`: off by default, and one
  log line the first time it replaces the pooling.
"""
from __future__ import annotations

import inspect
import logging
import os

import torch

from ..autograd import attach_pool, wants_grad
from ..vidcom2 import compress, compress_batch
from ._intercept import (batched_prefill_enabled, compressor_enabled, original_method, params_kwargs, retention_ratio,
                         shadow)
from ._prefill_prune import _DecodeLayout, _gather_slots, decode_state, run_decode_step, run_with_pruning
from .qwen2_5_vl import _cache_is_empty

__all__ = ["LlavaOnevisionModel_forward", "LlavaNextVideoModel_forward",
           "LlavaOnevisionForConditionalGeneration_forward", "LlavaNextVideoForConditionalGeneration_forward"]

_LOG = logging.getLogger(__name__)
_POOL_LOGGED = [False]


def _keep_indices(x: torch.Tensor, n: int, base_scale: float, stats_ws=None) -> torch.Tensor:
    """Kept token indices (ascending, int64) of one video's `[F*n, D]` tokens."""
    return compress(x, n, base_scale, "linear", gather=False, stats_ws=stats_ws, **params_kwargs()).global_idx


def _keep_indices_many(xs, n: int, base_scale: float):
    """`_keep_indices` of every row's video, all of them in flight (one host synchronisation for every count)."""
    return [r.global_idx for r in compress_batch(list(xs), n, base_scale, gather=False, **params_kwargs())]


def fused_pool_enabled() -> bool:
    """`VC2_FUSED_POOL=on` env knob (off by default for these hooks, unlike the `llava`-package hook)."""
    return os.getenv("VC2_FUSED_POOL", "") == "on"


def _fused_apply_pooling(self, clips: int, pooled: list):
    """OneVision's `apply_pooling`, replaced by pool + sweep 1 in one kernel (video by video: the statistics are per video)
    when the configuration allows a bit-identical pooled tensor; the model's own pooling otherwise."""
    inner = self.apply_pooling
    vision = self.config.vision_config
    side = vision.image_size // vision.patch_size

    def apply_pooling(image_features):
        x = image_features
        ok = (torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.shape[1] == side * side
              and x.dtype in (torch.float32, torch.bfloat16, torch.float16)
              and x.shape[-1] % (8 if x.dtype == torch.float32 else 16) == 0
              and 2 * ((side + 1) // 2) <= 128          # torch's other bilinear kernel beyond: another summation order
              and x.shape[0] % clips == 0)
        if not ok:
            return inner(image_features)
        from ..fused import pool_stats
        if not _POOL_LOGGED[0]:
            _POOL_LOGGED[0] = True
            _LOG.warning("vidcom2: VC2_FUSED_POOL=on -- apply_pooling of %s runs as vc2_pool_stats (torch's CPU bilinear "
                         "bits; may differ by rounding from the GPU interpolate)", type(self).__name__)
        frames = x.shape[0] // clips
        outs = []
        for b in range(clips):
            xb = x[b * frames:(b + 1) * frames]
            out, ws = pool_stats(xb, side, side, "bilinear")
            pooled.append((out.view(-1, out.shape[-1]), ws))        # (scored as is: the prompt gets a copy of it)
            if wants_grad(xb):
                # same forward bits; the backward is the model's own pooling Jacobian
                out = attach_pool(out, xb, inner)
            outs.append(out)
        return outs[0] if clips == 1 else torch.cat(outs)

    return apply_pooling


def _hooked_forward(self, hook, args, kwargs, newline: bool):
    original = original_method(self, "forward", hook)
    try:
        bound = inspect.signature(original).bind_partial(*args, **kwargs).arguments
    except TypeError:
        bound = dict(kwargs)
    bound = {**bound.get("kwargs", {}), **bound}
    prefill = _cache_is_empty(bound.get("past_key_values"))
    if prefill or not compressor_enabled():
        decode_state(self, clear=True)          # (a pruned prefill's layout lives until the next prefill)
    elif decode_state(self) is not None:
        # a decode step behind a pruned prefill: the KV cache holds the PRUNED prompt
        return run_decode_step(self, lambda: original(*args, **kwargs))
    videos = bound.get("pixel_values_videos")
    ref = bound.get("input_ids") if bound.get("input_ids") is not None else bound.get("inputs_embeds")
    active = (compressor_enabled() and torch.is_tensor(videos) and videos.dim() == 5 and prefill and ref is not None
              and (ref.shape[0] == 1 or batched_prefill_enabled()))
    if not active:
        return original(*args, **kwargs)

    clips, frames = int(videos.shape[0]), int(videos.shape[1])
    extra = 1 if newline else 0
    base_scale = retention_ratio()
    pooled: list = []                           # (fused pooling) per video: the pooled [F*n, D] tensor, its statistics

    def choose(video_embeds):
        """One ascending list over the prompts' video tokens (video features are in placeholder order): per video its
        kept tokens, then (OneVision) its newline ordinal.  None: not the layout this hook knows."""
        per_clip = video_embeds.shape[0] // clips
        if video_embeds.dim() != 2 or video_embeds.shape[0] != per_clip * clips or per_clip - extra <= 0 \
                or (per_clip - extra) % frames:
            return None
        n = (per_clip - extra) // frames
        xs = [video_embeds[c * per_clip: c * per_clip + frames * n] for c in range(clips)]
        one, many = globals()["_keep_indices"], globals()["_keep_indices_many"]
        if len(pooled) == clips:
            # the pooled tensors themselves are scored (same bits; the prompt holds a copy behind torch.cat): their
            # statistics are already in the workspace
            kept = [one(own, n, base_scale, ws) if own.shape == x.shape and own.dtype == x.dtype and own.device == x.device
                    else one(x, n, base_scale) for x, (own, ws) in zip(xs, pooled)]
        else:
            kept = [one(xs[0], n, base_scale)] if clips == 1 else many(xs, n, base_scale)
        out = []
        for c, idx in enumerate(kept):
            out.append(idx + c * per_clip)
            if newline:         # appended on the device, once the counts are known
                out.append(torch.full((1,), c * per_clip + frames * n, dtype=torch.int64, device=idx.device))
        return out[0] if len(out) == 1 else torch.cat(out)

    def choose_many(video_embeds):
        kept = choose(video_embeds)
        return torch.arange(video_embeds.shape[0], device=video_embeds.device) if kept is None else kept

    def run():
        return run_with_pruning(self, lambda: original(*args, **kwargs), choose, choose_many=choose_many, renumber=True)

    if newline and fused_pool_enabled():
        with shadow(self, apply_pooling=_fused_apply_pooling(self, clips, pooled)):
            out = run()
    else:
        out = run()
    st = self._vidcom2_last
    if st.pruned and st.decode is None:
        # B = 1: the decode steps see the prefill's pruned mask followed by the columns generate appends, and count
        # their positions on from S' (the batched layout leaves the same for B > 1)
        keep = st.keep_token_indices
        S, Sp = int(st.video_mask.shape[1]), int(keep.numel())
        am = bound.get("attention_mask")
        mask = (am[:, keep.to(am.device)] if torch.is_tensor(am) and am.dim() == 2
                else torch.ones((1, Sp), dtype=torch.int64, device=keep.device))
        self.__dict__["_vidcom2_decode"] = _DecodeLayout(mask, keep[None], S, torch.full((1,), S - Sp, dtype=torch.int64,
                                                                                  device=keep.device))
    return out


def _mirror_signature(hook, module: str, name: str) -> None:
    """`inspect.signature(hook)` shows the installed forward's parameters (HF generate validates its keyword arguments
    against them); the hook itself passes whatever it gets through to that forward."""
    try:
        import importlib
        hook.__signature__ = inspect.signature(getattr(importlib.import_module(module), name).forward)
    except Exception:           # (this transformers has no such class: the hook is never installed on one either)
        pass


def LlavaOnevisionModel_forward(self, *args, **kwargs):
    """Bound on a `LlavaOnevisionModel`; the parameter list is the installed class's (`_mirror_signature`)."""
    return _hooked_forward(self, LlavaOnevisionModel_forward, args, kwargs, newline=True)


def LlavaNextVideoModel_forward(self, *args, **kwargs):
    """Bound on a `LlavaNextVideoModel`; the parameter list is the installed class's (`_mirror_signature`)."""
    return _hooked_forward(self, LlavaNextVideoModel_forward, args, kwargs, newline=False)


_mirror_signature(LlavaOnevisionModel_forward, "transformers.models.llava_onevision.modeling_llava_onevision",
                  "LlavaOnevisionModel")
_mirror_signature(LlavaNextVideoModel_forward, "transformers.models.llava_next_video.modeling_llava_next_video",
                  "LlavaNextVideoModel")


def _outer_forward(self, hook, args, kwargs):
    """With `labels`, the outer forward runs without them and the model's own `loss_function` is applied to the logits
    of the pruned sequence, against the labels gathered with the same keep list (-100 in a batch's pad slots).  Without
    labels (generate) it is the outer forward, called as is."""
    original = original_method(self, "forward", hook)
    if not compressor_enabled():
        return original(*args, **kwargs)
    try:
        bound = inspect.signature(original).bind_partial(*args, **kwargs)
    except TypeError:
        return original(*args, **kwargs)
    call = bound.arguments
    labels = call.get("labels")
    if labels is None:
        return original(*args, **kwargs)
    call["labels"] = None
    extra = call.setdefault("kwargs", {})
    as_tuple = extra.pop("return_dict", None) is False
    loss_kwargs = dict(extra)
    extra["return_dict"] = True
    inner = self.model
    inner.__dict__.pop("_vidcom2_last", None)
    out = original(*bound.args, **bound.kwargs)
    st = inner.__dict__.get("_vidcom2_last")
    if st is not None and st.pruned:
        keep = st.keep_token_indices
        labels = (labels[:, keep.to(labels.device)] if keep.dim() == 1
                  else _gather_slots(labels, keep.to(labels.device), -100))
    loss = self.loss_function(logits=out.logits, labels=labels, vocab_size=self.config.get_text_config().vocab_size,
                              **loss_kwargs)
    out = type(out)(loss=loss, **{k: v for k, v in out.items() if k != "loss"})       # (loss first, as the model orders it)
    return out.to_tuple() if as_tuple else out


def LlavaOnevisionForConditionalGeneration_forward(self, *args, **kwargs):
    """Bound by `install()` on a `LlavaOnevisionForConditionalGeneration` (the labels path, `_outer_forward`)."""
    return _outer_forward(self, LlavaOnevisionForConditionalGeneration_forward, args, kwargs)


def LlavaNextVideoForConditionalGeneration_forward(self, *args, **kwargs):
    """Bound by `install()` on a `LlavaNextVideoForConditionalGeneration` (the labels path, `_outer_forward`)."""
    return _outer_forward(self, LlavaNextVideoForConditionalGeneration_forward, args, kwargs)


_mirror_signature(LlavaOnevisionForConditionalGeneration_forward,
                  "transformers.models.llava_onevision.modeling_llava_onevision", "LlavaOnevisionForConditionalGeneration")
_mirror_signature(LlavaNextVideoForConditionalGeneration_forward,
                  "transformers.models.llava_next_video.modeling_llava_next_video",
                  "LlavaNextVideoForConditionalGeneration")

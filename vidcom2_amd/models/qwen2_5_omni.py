"""Qwen2.5-Omni hook: video-token pruning in the thinker's prefill.

    thinker.forward = types.MethodType(Qwen2_5OmniThinker_forward, thinker)     # or vidcom2_amd.models.install(model)

Provenance: the reference's Omni hooks live on an upstream branch that is not part of the reference checkout.  The
semantics here are the reference's Qwen2.5-VL hook (token_compressor/vidcom2/models/qwen2_5_vl.py:20-202) applied to
the thinker, and its Qwen3-VL hook for the deep-stack part (qwen3_vl.py) -- pinned against the oracle's stage chain,
like the Qwen2-VL row, not against a golden of a reference Omni hook.

What the hook does, on top of the shared interceptor (`_prefill_prune.py`, `lm_attr="model"`: the thinker calls
`self.model`, not `self.language_model`):

* same gating as the Qwen-VL hooks (`COMPRESSOR=vidcom2`, video inputs present, empty KV cache, B = 1 or
  `VC2_BATCHED_PREFILL=1`); otherwise the thinker's own forward runs untouched;
* every video is scored on its own (`_compute_keep_indices` / `_compute_keep_indices_many`); only video placeholder
  positions are dropped -- text, image and audio tokens stay, including the audio chunks `use_audio_in_video=True`
  interleaves between a video's frames.  The TMRoPE positions the thinker computes on the unpruned prompt are sliced;
* decode positions: the thinker numbers decode steps `past_key_values.get_seq_length() + self.rope_deltas`.  After a
  pruned prefill the cache holds S' < S entries, so `rope_deltas` is shifted by S - S' (one shift for every row: B > 1
  rows are re-padded to one length S') and generation continues at the unpruned prompt's positions.  The decode-step
  attention mask generate grows for the unpruned prompt is mapped onto the pruned cache (`run_decode_step`);
* `labels` are cut with the same keep list (-100 in the pad slots of a batch) and the loss is taken over the pruned
  sequence;
* installed through the outer `*OmniForConditionalGeneration`, a `generate` that asks for audio output (explicitly or
  by the `has_talker` default) runs the thinker unpruned with one `RuntimeWarning`: the talker reads the thinker's
  prompt hidden states next to the unpruned `input_ids`.  Pruning for the talker is not supported.
"""
from __future__ import annotations

import inspect
import sys
import warnings

import torch

from ._intercept import batched_prefill_enabled, compressor_enabled, original_method, retention_ratio, shadow
from ._prefill_prune import _DecodeLayout, _gather_slots, decode_state, run_decode_step, run_with_pruning
from .qwen2_5_vl import _cache_is_empty, _keep_per_video, named_call_kwargs

__all__ = ["Qwen2_5OmniThinker_forward", "install_outer"]

_AUDIO_OUT = "_vidcom2_audio_out"        # set on the thinker while the outer generate feeds the talker


def omni_thinker_forward(self, hook, named: dict, extra: dict):
    """Shared by the Qwen2.5-Omni and Qwen3-Omni thinker hooks."""
    from . import qwen2_5_vl as Q              # (the scoring functions are looked up at call time: tests replace them)
    kwargs = named_call_kwargs(self, hook, named, extra)
    original = original_method(self, "forward", hook)
    prefill = _cache_is_empty(kwargs.get("past_key_values"))
    if prefill or not compressor_enabled():
        decode_state(self, clear=True)
    elif decode_state(self) is not None:
        # a decode step behind a pruned prefill: the KV cache holds the PRUNED prompt
        return run_decode_step(self, lambda: original(**kwargs), lm_attr="model")
    video_grid_thw = kwargs.get("video_grid_thw")
    ref = kwargs.get("input_ids") if kwargs.get("input_ids") is not None else kwargs.get("inputs_embeds")
    active = (compressor_enabled() and kwargs.get("pixel_values_videos") is not None and video_grid_thw is not None
              and prefill and ref is not None and not self.__dict__.get(_AUDIO_OUT, False)
              and (ref.shape[0] == 1 or batched_prefill_enabled()))
    if not active:
        return original(**kwargs)

    merge_size = self.visual.spatial_merge_size
    base_scale = retention_ratio()

    def choose(video_embeds):
        return _keep_per_video(video_embeds, video_grid_thw, merge_size, base_scale, Q._compute_keep_indices)

    def choose_many(video_embeds):
        split_sizes = (video_grid_thw.prod(-1) // merge_size ** 2).tolist()
        return Q._compute_keep_indices_many(torch.split(video_embeds, split_sizes), video_grid_thw, merge_size,
                                            base_scale)

    labels = kwargs.pop("labels", None)
    as_tuple = kwargs.pop("return_dict", True) is False
    router = _router_requested(self, original, kwargs)
    if router:
        # the thinker would weigh the router logits of the S' kept tokens with its UNPRUNED [B, S] mask: it skips the
        # router term, the decoder still records the logits, and the term is taken below with the mask they go with
        kwargs["output_router_logits"] = False
        router = _RouterCapture(self.model)
        with shadow(self, model=router):
            out = run_with_pruning(self, lambda: original(**kwargs), choose, lm_attr="model", choose_many=choose_many)
        out["aux_loss"] = _router_loss(self, router)
    else:
        out = run_with_pruning(self, lambda: original(**kwargs), choose, lm_attr="model", choose_many=choose_many)
    st = self._vidcom2_last
    if st.pruned:
        keep = st.keep_token_indices
        S, Sp = int(st.video_mask.shape[1]), int(keep.shape[-1])
        if self.rope_deltas is not None and S != Sp:
            self.rope_deltas = self.rope_deltas + (S - Sp)
            if getattr(out, "rope_deltas", None) is not None:
                out.rope_deltas = self.rope_deltas
        am = kwargs.get("attention_mask")
        if st.decode is None and torch.is_tensor(am) and am.dim() == 2 and am.shape[0] == 1:
            # B = 1: the decode steps see the prefill's pruned mask followed by the columns generate appends
            self.__dict__["_vidcom2_decode"] = _DecodeLayout(am[:, keep.to(am.device)], keep[None], S)
        if labels is not None:
            labels = (labels[:, keep.to(labels.device)] if keep.dim() == 1
                      else _gather_slots(labels, keep.to(labels.device), -100))
    if labels is not None:
        out["loss"] = _loss(self, out, labels)
    return out.to_tuple() if as_tuple else out


def _loss(self, out, labels):
    """The thinker's own loss (its forward: `self.loss_function(...)`, plus the router term for Qwen3-Omni), over the
    logits of the pruned sequence."""
    loss = self.loss_function(logits=out.logits, labels=labels, vocab_size=self.config.get_text_config().vocab_size)
    aux = getattr(out, "aux_loss", None)
    if aux is not None:
        loss = loss + self.router_aux_loss_coef * aux.to(loss.device)
    return loss


def _router_requested(self, original, kwargs) -> bool:
    """Whether the thinker (Qwen3-Omni: an MoE decoder) will add the router load-balancing term: its
    `output_router_logits` argument, the text config's default when None."""
    if "output_router_logits" not in inspect.signature(original).parameters:
        return False
    flag = kwargs.get("output_router_logits")
    return bool(self.config.get_text_config().output_router_logits if flag is None else flag)


class _RouterCapture:
    """Stands in for the thinker's decoder stack during one forward: asks it for the router logits and keeps them,
    with the attention mask they were computed under (the pruned one when the interceptor cut the prompt)."""

    def __init__(self, real):
        self._real, self.router_logits, self.mask = real, None, None

    def __getattr__(self, name):
        return getattr(self.__dict__["_real"], name)

    def __call__(self, *args, **kwargs):
        kwargs["output_router_logits"] = True
        out = self._real(*args, **kwargs)
        am = kwargs.get("attention_mask")
        self.router_logits, self.mask = out.router_logits, am if torch.is_tensor(am) and am.dim() == 2 else None
        return out


def _router_loss(self, router: _RouterCapture):
    """The thinker's `load_balancing_loss_func` (its own module's) over the tokens the decoder saw."""
    balance = sys.modules[type(self).__module__].load_balancing_loss_func
    return balance(router.router_logits, self.num_experts, self.num_experts_per_tok, router.mask)


def _audio_requested(outer, args, kwargs) -> bool:
    """Whether the outer generate will run the talker: upstream's rule for both families (Qwen2.5-Omni:
    `generation_mode` / the deprecated `return_audio`; Qwen3-Omni: `return_audio`), None meaning `has_talker`."""
    mode = kwargs.get("generation_mode", kwargs.get("return_audio"))
    if mode is None and args:
        try:
            mode = inspect.signature(original_method(outer, "generate", _outer_generate)).bind_partial(
                *args, **kwargs).arguments.get("return_audio")
        except TypeError:
            mode = None
    talker = bool(getattr(outer, "has_talker", False))
    return talker if mode is None else (talker and mode is not False and mode != "text")


def _outer_generate(self, *args, **kwargs):
    generate = original_method(self, "generate", _outer_generate)
    if compressor_enabled() and _audio_requested(self, args, kwargs):
        warnings.warn("vidcom2: audio output reads the thinker's prompt hidden states next to the unpruned input_ids; "
                      "this generate runs the thinker unpruned", RuntimeWarning, stacklevel=2)
        with shadow(self.thinker, **{_AUDIO_OUT: True}):
            return generate(*args, **kwargs)
    return generate(*args, **kwargs)


def install_outer(model, hook) -> None:
    """Bind `hook` on `model.thinker` and the audio-output gate on the outer model's `generate`."""
    import types
    model.thinker.__dict__["forward"] = types.MethodType(hook, model.thinker)
    model.__dict__["generate"] = types.MethodType(_outer_generate, model)


def Qwen2_5OmniThinker_forward(
    self,
    input_ids=None,
    input_features=None,
    pixel_values=None,
    pixel_values_videos=None,
    image_grid_thw=None,
    video_grid_thw=None,
    attention_mask=None,
    feature_attention_mask=None,
    audio_feature_lengths=None,
    position_ids=None,
    past_key_values=None,
    inputs_embeds=None,
    labels=None,
    use_cache=None,
    use_audio_in_video=None,
    video_second_per_grid=None,
    **kwargs,
):
    """The parameter list of `Qwen2_5OmniThinkerForConditionalGeneration.forward`."""
    named = dict(input_ids=input_ids, input_features=input_features, pixel_values=pixel_values,
                 pixel_values_videos=pixel_values_videos, image_grid_thw=image_grid_thw, video_grid_thw=video_grid_thw,
                 attention_mask=attention_mask, feature_attention_mask=feature_attention_mask,
                 audio_feature_lengths=audio_feature_lengths, position_ids=position_ids,
                 past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels, use_cache=use_cache,
                 use_audio_in_video=use_audio_in_video, video_second_per_grid=video_second_per_grid)
    return omni_thinker_forward(self, Qwen2_5OmniThinker_forward, named, kwargs)

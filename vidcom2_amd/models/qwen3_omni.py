"""Qwen3-Omni hook: video-token pruning in the thinker's prefill.

    thinker.forward = types.MethodType(Qwen3OmniMoeThinker_forward, thinker)    # or vidcom2_amd.models.install(model)

Same gating, scoring, pruning, decode-position shift, label cut and audio-output gate as the Qwen2.5-Omni hook
(`qwen2_5_omni.py`, which also states the provenance).  In addition the deep-stack features travel with the visual
tokens, so `visual_pos_masks` and every layer of `deepstack_visual_embeds` are cut to the kept positions, as for
Qwen3-VL (reference: token_compressor/vidcom2/models/qwen3_vl.py).  The thinker's TMRoPE positions are fp32 here; they
are sliced, never rounded.
"""
from __future__ import annotations

from .qwen2_5_omni import omni_thinker_forward

__all__ = ["Qwen3OmniMoeThinker_forward"]


def Qwen3OmniMoeThinker_forward(
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
    output_router_logits=None,
    use_audio_in_video=None,
    video_second_per_grid=None,
    **kwargs,
):
    """The parameter list of `Qwen3OmniMoeThinkerForConditionalGeneration.forward`."""
    named = dict(input_ids=input_ids, input_features=input_features, pixel_values=pixel_values,
                 pixel_values_videos=pixel_values_videos, image_grid_thw=image_grid_thw, video_grid_thw=video_grid_thw,
                 attention_mask=attention_mask, feature_attention_mask=feature_attention_mask,
                 audio_feature_lengths=audio_feature_lengths, position_ids=position_ids,
                 past_key_values=past_key_values, inputs_embeds=inputs_embeds, labels=labels, use_cache=use_cache,
                 output_router_logits=output_router_logits, use_audio_in_video=use_audio_in_video,
                 video_second_per_grid=video_second_per_grid)
    return omni_thinker_forward(self, Qwen3OmniMoeThinker_forward, named, kwargs)

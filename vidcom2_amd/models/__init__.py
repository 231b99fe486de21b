"""Model hooks: the reference's `token_compressor/vidcom2/models/` surface.

    from vidcom2_amd.models.llava import cus_prepare_inputs_labels_for_multimodal
    from vidcom2_amd.models.qwen2_5_vl import Qwen2_5_VLModel_forward
    from vidcom2_amd.models.qwen2_vl import Qwen2VL_ViT_forward, Qwen2VLGeneration_forward
    from vidcom2_amd.models.qwen3_vl import Qwen3VLModel_forward
    from vidcom2_amd.models.qwen2_5_omni import Qwen2_5OmniThinker_forward
    from vidcom2_amd.models.qwen3_omni import Qwen3OmniMoeThinker_forward
    from vidcom2_amd.models.llava_hf import LlavaOnevisionModel_forward, LlavaNextVideoModel_forward

Same names, same installation (`types.MethodType(hook, model)`), same env knobs (`COMPRESSOR`,
`R_RATIO`); implemented as wrappers around the installed model's own methods, see `_intercept.py`.
The two Omni hooks (Qwen2.5-Omni, Qwen3-Omni) sit on the thinker's `forward`; their semantics are the Qwen2.5-VL /
Qwen3-VL hooks applied to the thinker (the reference's Omni hooks are not in its checkout, see `qwen2_5_omni.py`).
The two `llava_hf` hooks sit on transformers' `LlavaOnevisionModel` / `LlavaNextVideoModel` (the reference hooks the
LLaVA-NeXT package only); their semantics are the `one_token` branch of the reference's LLaVA hook, see `llava_hf.py`.
"""
from __future__ import annotations

import types

from ._intercept import compressor_enabled

__all__ = ["install"]


def install(model, force: bool = False) -> bool:
    """Bind the matching hook on `model` the way the reference's lmms-eval wrappers do
    (lmms_eval/models/llava_onevision.py:157-163, README.md:76-93): only when `COMPRESSOR=vidcom2`
    (or `force`), with `types.MethodType`.  Returns whether a hook was bound.

    LLaVA-OneVision / LLaVA-Video : `model.prepare_inputs_labels_for_multimodal` (the LLaVA-NeXT `llava` package)
    transformers' LlavaOnevision* / LlavaNextVideo* : `forward` of the inner `*Model`; a `*ForConditionalGeneration`
                                    also gets the labels wrapper on its own `forward`
    Qwen2.5-VL / Qwen2-VL / Qwen3-VL : `forward` of the inner `*Model` (`model.model` of a
                                    `*ForConditionalGeneration`)
    Qwen2.5-Omni / Qwen3-Omni      : `forward` of the thinker (`model.thinker` of the outer model, which also gets
                                    the audio-output gate on its `generate`; or the bare thinker)
    """
    if not (force or compressor_enabled()):
        return False
    names = {k.__name__ for k in type(model).__mro__}
    if hasattr(model, "prepare_inputs_labels_for_multimodal"):
        from .llava import cus_prepare_inputs_labels_for_multimodal as hook
        model.__dict__["prepare_inputs_labels_for_multimodal"] = types.MethodType(hook, model)
        return True
    omni = _omni_hook(names)
    if omni is not None and hasattr(model, "thinker"):
        from .qwen2_5_omni import install_outer
        install_outer(model, omni)
        return True
    if omni is not None and any(n.endswith("ThinkerForConditionalGeneration") for n in names):
        model.__dict__["forward"] = types.MethodType(omni, model)
        return True
    inner = model.model if any(n.endswith("ForConditionalGeneration") for n in names) else model
    inner_names = {k.__name__ for k in type(inner).__mro__}
    outer = None
    if any(n.startswith("LlavaOnevision") for n in inner_names):
        from .llava_hf import LlavaOnevisionForConditionalGeneration_forward as outer
        from .llava_hf import LlavaOnevisionModel_forward as hook
    elif any(n.startswith("LlavaNextVideo") for n in inner_names):
        from .llava_hf import LlavaNextVideoForConditionalGeneration_forward as outer
        from .llava_hf import LlavaNextVideoModel_forward as hook
    elif any(n.startswith("Qwen3VL") for n in inner_names):
        from .qwen3_vl import Qwen3VLModel_forward as hook
    elif any(n.startswith("Qwen2_5_VL") for n in inner_names):
        from .qwen2_5_vl import Qwen2_5_VLModel_forward as hook
    elif any(n.startswith("Qwen2VL") for n in inner_names):
        from .qwen2_vl import Qwen2VLModel_forward as hook
    else:
        raise TypeError(f"vidcom2_amd.models.install: no hook for {type(model).__name__}")
    inner.__dict__["forward"] = types.MethodType(hook, inner)
    if outer is not None and inner is not model:
        model.__dict__["forward"] = types.MethodType(outer, model)         # (labels: the loss over the pruned sequence)
    return True


def _omni_hook(names):
    if any(n.startswith("Qwen3OmniMoe") for n in names):
        from .qwen3_omni import Qwen3OmniMoeThinker_forward
        return Qwen3OmniMoeThinker_forward
    if any(n.startswith("Qwen2_5Omni") for n in names):
        from .qwen2_5_omni import Qwen2_5OmniThinker_forward
        return Qwen2_5OmniThinker_forward
    return None

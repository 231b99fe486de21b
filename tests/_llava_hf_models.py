"""Tiny random-weight LLaVA-OneVision / LLaVA-NeXT-Video models of the installed transformers and their prompts (test
infrastructure for test_llava_hf_hooks.py).

* "onevision": SigLIP tower (hidden 32, 1 layer, image 54 / patch 2 -> 27x27 patches, pooled bilinearly to the real
  14x14 = 196 tokens per frame) + Qwen2 text (hidden 64, 2 layers);
* "next_video": CLIP tower (hidden 32, 1 layer, image 24 / patch 2 -> 12x12 patches, average-pooled to 36 tokens per
  frame) + Llama text (hidden 64, 2 layers).

Token ids live in the small vocabulary of `_stub_models` (text 1..50, pad 0, image 60, video 61).  The CPU tests run the
real towers on random pixels; the GPU tests inject synthetic features (`set_video_features`, as
`_stub_models.set_video_features` does for the Qwen-VL tests) so that the inputs are bit-portable.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import _stub_models as S

FAMILIES = ["onevision", "next_video"]
D = 64
IMG = {"onevision": 54, "next_video": 24}
TPF = {"onevision": 196, "next_video": 36}              # pooled tokens per frame
NEWLINE = {"onevision": True, "next_video": False}      # one image_newline row behind a video's tokens


def config(family: str, hidden: int = D, layers: int = 2):
    text = dict(vocab_size=S.VOCAB, hidden_size=hidden, intermediate_size=64, num_hidden_layers=layers,
                num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=8192, bos_token_id=1,
                eos_token_id=2, pad_token_id=0)
    vision = dict(hidden_size=32, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2,
                  image_size=IMG[family], patch_size=2)
    side = IMG[family]
    if family == "onevision":
        from transformers.models.llava_onevision import LlavaOnevisionConfig
        return LlavaOnevisionConfig(vision_config=dict(vision, model_type="siglip_vision_model", vision_use_head=False),
                                    text_config=dict(text, model_type="qwen2"), image_token_id=S.IMAGE_ID,
                                    video_token_id=S.VIDEO_ID, vision_feature_layer=-1,
                                    vision_feature_select_strategy="full", image_grid_pinpoints=[[side, side]],
                                    tie_word_embeddings=False)
    from transformers.models.llava_next_video import LlavaNextVideoConfig
    return LlavaNextVideoConfig(vision_config=dict(vision, model_type="clip_vision_model", projection_dim=32),
                                text_config=dict(text, model_type="llama"), image_token_index=S.IMAGE_ID,
                                video_token_index=S.VIDEO_ID, vision_feature_layer=-1,
                                vision_feature_select_strategy="default", image_grid_pinpoints=[[side, side]],
                                spatial_pool_stride=2, spatial_pool_mode="average", tie_word_embeddings=False)


def classes(family: str):
    """(outer `*ForConditionalGeneration`, inner `*Model`) of the installed transformers."""
    if family == "onevision":
        from transformers.models.llava_onevision.modeling_llava_onevision import (
            LlavaOnevisionForConditionalGeneration, LlavaOnevisionModel)
        return LlavaOnevisionForConditionalGeneration, LlavaOnevisionModel
    from transformers.models.llava_next_video.modeling_llava_next_video import (
        LlavaNextVideoForConditionalGeneration, LlavaNextVideoModel)
    return LlavaNextVideoForConditionalGeneration, LlavaNextVideoModel


def model(family: str, dtype=torch.float32, device="cpu", outer: bool = True, hidden: int = D, layers: int = 2):
    """The same weights on every call (seed 0), eval mode."""
    Outer, Inner = classes(family)
    torch.manual_seed(0)
    m = (Outer if outer else Inner)(config(family, hidden, layers)).eval()
    return m.to(device=device, dtype=dtype)


def image_tokens(inner) -> int:
    """Placeholders one square image takes (anyres: the base patch and one grid patch, unpadded, with newlines)."""
    family = "onevision" if type(inner).__name__.startswith("LlavaOnevision") else "next_video"
    side = IMG[family]
    p = next(inner.parameters())
    cfg = inner.config
    with torch.no_grad():
        out = inner.get_image_features(torch.zeros(1, 2, 3, side, side, dtype=p.dtype, device=p.device),
                                       torch.tensor([[side, side]]), vision_feature_layer=cfg.vision_feature_layer,
                                       vision_feature_select_strategy=cfg.vision_feature_select_strategy,
                                       return_dict=True).pooler_output
    return int(sum(t.shape[0] for t in out))


def prompt(family: str, frames: int, seed: int, prefix: int = 6, suffix: int = 5, n_image: int = 0, video: bool = True,
           dtype=torch.float32, pixels: bool = True):
    """text + [one image of n_image placeholders + text] + [one video] + text -> kwargs of the model's forward.
    pixels=False: the video is a [1, frames, 1, 1, 1] dummy (features injected with `set_video_features`)."""
    side, n = IMG[family], TPF[family]
    g = torch.Generator().manual_seed(seed)
    parts = [S.text_ids(prefix, seed)]
    kw = {}
    if n_image:
        parts += [torch.full((n_image,), S.IMAGE_ID), S.text_ids(2, seed + 300)]
        kw.update(pixel_values=torch.randn(1, 2, 3, side, side, generator=g).to(dtype),
                  image_sizes=torch.tensor([[side, side]]))
    if video:
        parts.append(torch.full((frames * n + (1 if NEWLINE[family] else 0),), S.VIDEO_ID))
        kw["pixel_values_videos"] = (torch.randn(1, frames, 3, side, side, generator=g).to(dtype) if pixels
                                     else torch.zeros(1, frames, 1, 1, 1, dtype=dtype))
    parts.append(S.text_ids(suffix, seed + 7))
    ids = torch.cat([p.to(torch.int64) for p in parts])[None]
    return dict(input_ids=ids, attention_mask=torch.ones_like(ids), **kw)


def batch(rows, side: str = "left"):
    """Prompts of different lengths (every one with a video of the same frame count) as one padded batch."""
    L = max(r["input_ids"].shape[1] for r in rows)
    ids = torch.zeros(len(rows), L, dtype=torch.int64)
    mask = torch.zeros(len(rows), L, dtype=torch.int64)
    for b, r in enumerate(rows):
        m = r["input_ids"].shape[1]
        sl = slice(L - m, L) if side == "left" else slice(0, m)
        ids[b, sl], mask[b, sl] = r["input_ids"][0], 1
    kw = dict(input_ids=ids, attention_mask=mask,
              pixel_values_videos=torch.cat([r["pixel_values_videos"] for r in rows]))
    if any("pixel_values" in r for r in rows):
        kw.update(pixel_values=torch.cat([r["pixel_values"] for r in rows if "pixel_values" in r]),
                  image_sizes=torch.cat([r["image_sizes"] for r in rows if "image_sizes" in r]))
    return kw


def to_device(kw, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in kw.items()}


def set_video_features(inner, family: str, feats):
    """Make the video tower + projector (+ pooling) deliver `feats`: one [F, n, D] tensor per video."""
    if family == "onevision":
        out = SimpleNamespace(pooler_output=torch.stack([f.reshape(-1, f.shape[-1]) for f in feats]))
    else:
        out = SimpleNamespace(pooler_output=tuple(feats))
    inner.__dict__["get_video_features"] = lambda *a, **k: out


def record(inner):
    """Keyword arguments of every call into the decoder stack."""
    calls = []
    inner.language_model.register_forward_pre_hook(lambda mod, args, kw: calls.append(dict(kw)), with_kwargs=True)
    return calls

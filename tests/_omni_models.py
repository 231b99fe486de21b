"""Tiny random-weight Qwen2.5-Omni / Qwen3-Omni thinkers and their prompts (test infrastructure).

The thinkers are the installed transformers' real classes with a small config: real decoder stack, real TMRoPE
(`get_rope_index`), real placeholder masks.  Their towers are built but bypassed: `get_video_features`,
`get_image_features` and `get_audio_features` are replaced on the instance so that the prompt carries synthetic
features from `vidcom2_amd.synth` (bit-portable), as `_stub_models.set_video_features` does for the Qwen-VL tests.

Token ids live in the small vocabulary of `_stub_models` (text 1..50, pad 0).  With `use_audio_in_video=True` a
video's audio track is interleaved with its frames the way each family's `get_rope_index` orders them (Qwen2.5-Omni:
by time chunk; Qwen3-Omni: by position), so the video positions of a prompt are not contiguous.
"""
from __future__ import annotations

from types import SimpleNamespace

import torch

import _stub_models as S
from vidcom2_amd import synth

D = 64
VS, VE, AS, AE, AUDIO_ID = 55, 56, 57, 58, 62          # vision start / end, audio start / end, audio placeholder
PPS = 4                                                 # position_id_per_seconds (4 positions per second of video)
MEL = 8                                                 # mel bins of the (bypassed) audio tower


def thinker(family: str, dtype=torch.float32, device="cpu", layers: int = 2):
    """family in {"qwen2_5_omni", "qwen3_omni"} -> the thinker, eval mode."""
    rope = dict(rope_type="default", mrope_section=[4, 6, 6], rope_theta=10000.0)
    text = dict(vocab_size=S.VOCAB, hidden_size=D, intermediate_size=64, num_hidden_layers=layers,
                num_attention_heads=2, num_key_value_heads=2, max_position_embeddings=4096, bos_token_id=1,
                eos_token_id=2, pad_token_id=0, rope_parameters=rope)
    audio = dict(num_mel_bins=MEL, encoder_layers=1, encoder_attention_heads=2, encoder_ffn_dim=32, d_model=32,
                 output_dim=D)
    ids = dict(image_token_id=S.IMAGE_ID, video_token_id=S.VIDEO_ID, audio_token_id=AUDIO_ID,
               audio_start_token_id=AS, position_id_per_seconds=PPS)
    if family == "qwen2_5_omni":
        from transformers.models.qwen2_5_omni import Qwen2_5OmniThinkerConfig as Cfg
        from transformers.models.qwen2_5_omni.modeling_qwen2_5_omni import \
            Qwen2_5OmniThinkerForConditionalGeneration as Model
        vision = dict(depth=1, hidden_size=32, intermediate_size=32, num_heads=2, out_hidden_size=D,
                      fullatt_block_indexes=[0], spatial_merge_size=2)
        cfg = Cfg(text_config=text, vision_config=vision, audio_config=audio, seconds_per_chunk=1,
                  audio_end_token_id=AE, **{k.replace("_id", "_index") if k in ("image_token_id", "video_token_id",
                                                                                 "audio_token_id") else k: v
                                            for k, v in ids.items()})
    else:
        from transformers.models.qwen3_omni_moe import Qwen3OmniMoeThinkerConfig as Cfg
        from transformers.models.qwen3_omni_moe.modeling_qwen3_omni_moe import \
            Qwen3OmniMoeThinkerForConditionalGeneration as Model
        text.update(head_dim=32, num_experts=4, num_experts_per_tok=2, moe_intermediate_size=32,
                    rope_parameters=dict(rope, mrope_interleaved=True))
        vision = dict(depth=1, hidden_size=32, intermediate_size=32, num_heads=2, out_hidden_size=D,
                      spatial_merge_size=2, deepstack_visual_indexes=[0], num_position_embeddings=16)
        cfg = Cfg(text_config=text, vision_config=vision, audio_config=audio, **ids)
    cfg.vision_start_token_id, cfg.vision_end_token_id, cfg.audio_end_token_id = VS, VE, AE
    torch.manual_seed(0)
    return Model(cfg).eval().to(device=device, dtype=dtype)


def audio_tokens(family: str, n_feat: int) -> int:
    """Tokens the thinker's TMRoPE gives an audio of n_feat mel frames (its `get_rope_index`)."""
    if family == "qwen2_5_omni":
        return ((n_feat - 1) // 2 + 1 - 2) // 2 + 1
    from transformers.models.qwen3_omni_moe.modeling_qwen3_omni_moe import _get_feat_extract_output_lengths
    return int(_get_feat_extract_output_lengths(torch.tensor(n_feat), 50))


def _interleave(family: str, frames: int, per_frame: int, n_audio: int):
    """Token order of a video with its audio track: list of ("v", n) / ("a", n) runs."""
    runs = []
    if family == "qwen2_5_omni":                      # chunks of PPS positions (seconds_per_chunk = 1): v0 a0 v1 a1 ...
        n_chunks = max(frames, -(-n_audio // PPS))
        for j in range(n_chunks):
            if j < frames:
                runs.append(("v", per_frame))
            a = min(PPS, n_audio - j * PPS)
            if a > 0:
                runs.append(("a", a))
    else:                                            # merged by position: frame t at PPS * t, audio token k at k
        a = 0
        for t in range(frames):
            take = min(max(PPS * t - a, 0), n_audio - a)
            if take:
                runs.append(("a", take))
                a += take
            runs.append(("v", per_frame))
        if a < n_audio:
            runs.append(("a", n_audio - a))
    return runs


def prompt(family: str, grids, seed: int, audio_in_video: bool, n_image_grid=None, audio_feat: int = 40,
           prefix: int = 5, suffix: int = 4, dtype=torch.float32, deep_layers: int = 0):
    """One prompt: text, [image], videos (with their audio tracks when audio_in_video), text.
    Returns dict(ids [1, L], video feats (list), image feats (list), audio feats [n, D] or None, grids, kwargs for the
    thinker's forward, deep (Qwen3: per-layer deep-stack features of video / image))."""
    parts = [S.text_ids(prefix, seed)]
    vfeats, ifeats, afeats = [], [], []
    if n_image_grid is not None:
        t, h, w = n_image_grid
        n = t * (h * w) // 4
        ifeats.append(synth.to_torch(synth.gauss(seed + 500, 43, 0, n * D).reshape(n, D), dtype))
        parts += [torch.tensor([VS]), torch.full((n,), S.IMAGE_ID), torch.tensor([VE]), S.text_ids(2, seed + 300)]
    n_audio_tok = audio_tokens(family, audio_feat)
    for i, (t, h, w) in enumerate(grids):
        per = (h * w) // 4
        vfeats.append(S.video_feats(t, per, D, dtype, seed + i).reshape(t * per, D))
        if i:
            parts.append(S.text_ids(3, seed + 100 + i))
        if audio_in_video:
            parts += [torch.tensor([VS, AS])]
            for kind, n in _interleave(family, t, per, n_audio_tok):
                parts.append(torch.full((n,), S.VIDEO_ID if kind == "v" else AUDIO_ID))
            parts += [torch.tensor([AE, VE])]
            afeats.append(synth.to_torch(synth.gauss(seed + 700 + i, 45, 0, n_audio_tok * D).reshape(n_audio_tok, D),
                                         dtype))
        else:
            parts += [torch.tensor([VS]), torch.full((t * per,), S.VIDEO_ID), torch.tensor([VE])]
    parts.append(S.text_ids(suffix, seed + 7))
    ids = torch.cat([p.to(torch.int64) for p in parts])[None]
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), use_audio_in_video=audio_in_video)
    if grids:
        kw.update(pixel_values_videos=torch.zeros(1, 4), video_grid_thw=torch.tensor(grids),
                  video_second_per_grid=torch.ones(len(grids)))
    if n_image_grid is not None:
        kw.update(pixel_values=torch.zeros(1, 4), image_grid_thw=torch.tensor([n_image_grid]))
    if afeats:
        kw.update(input_features=torch.zeros(len(afeats), MEL, audio_feat),
                  feature_attention_mask=torch.ones(len(afeats), audio_feat, dtype=torch.int64))
    deep = None
    if deep_layers:
        nv = sum(f.shape[0] for f in vfeats)
        ni = sum(f.shape[0] for f in ifeats)
        deep = dict(video=S.deepstack_feats(nv, D, dtype, seed + 77, deep_layers),
                    image=S.deepstack_feats(ni, D, dtype, seed + 88, deep_layers) if ni else None)
    return dict(ids=ids, video=vfeats, image=ifeats, audio=torch.cat(afeats) if afeats else None, kw=kw, deep=deep)


def set_features(model, p, device=None):
    """Make the thinker's towers deliver the prompt's synthetic features."""
    dev = device or next(model.parameters()).device
    to = lambda ts: None if ts is None else [t.to(dev) for t in ts]          # noqa: E731
    deep = p["deep"] or {}
    S.set_video_features(model, to(p["video"]), to(deep.get("video")))
    if p["image"]:
        S.set_image_features(model, to(p["image"]), to(deep.get("image")))
    if p["audio"] is not None:
        out = SimpleNamespace(last_hidden_state=p["audio"].to(dev))
        model.__dict__["get_audio_features"] = lambda *a, **k: out


def to_device(kw, device):
    return {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in kw.items()}

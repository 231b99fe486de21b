#!/usr/bin/env python
"""One Qwen2.5-Omni thinker prefill, hooked (video tokens pruned) against unhooked.  Random weights at
Qwen2.5-Omni-7B text width (D = 3584, its MLP width and heads) with few decoder layers and a small vocabulary; one
64-frame video (196 tokens per frame) with its 64 s audio track interleaved (`use_audio_in_video=True`, 1600 audio
tokens), bf16.  The towers are bypassed: the prompt carries synthetic video / audio features, so the times are the
pruning step plus the decoder stack and lm_head.  Prints one JSON line (hipEvent medians):

  unhooked_ms / hooked_ms   thinker forward, prefill (use_cache=True), without / with the hook
  S / S_pruned              prompt length before / after pruning

    python scripts/omni_prefill.py [--layers 4] [--steps 10] [--warmup 3] [--ratio 0.25]
"""
import argparse
import json
import os
import sys
import types
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vidcom2_amd import synth                                                   # noqa: E402
from vidcom2_amd.models.qwen2_5_omni import Qwen2_5OmniThinker_forward          # noqa: E402

D, FRAMES, HW, PPS, CHUNK = 3584, 64, 28, 25, 2            # width, frames, patches per side, TMRoPE positions / s, s
VOCAB, TEXT_ID, VS, VE, AS, AE, VIDEO_ID, AUDIO_ID = 8192, 100, 8000, 8001, 8002, 8003, 8004, 8005
PER_FRAME = (HW // 2) ** 2
N_FEAT = 6400                                              # mel frames of 64 s -> 1600 audio tokens


def thinker(layers, dev):
    from transformers.models.qwen2_5_omni import Qwen2_5OmniThinkerConfig
    from transformers.models.qwen2_5_omni.modeling_qwen2_5_omni import Qwen2_5OmniThinkerForConditionalGeneration
    text = dict(vocab_size=VOCAB, hidden_size=D, intermediate_size=18944, num_hidden_layers=layers,
                num_attention_heads=28, num_key_value_heads=4, max_position_embeddings=32768,
                rope_parameters=dict(rope_type="default", mrope_section=[16, 24, 24], rope_theta=1000000.0))
    cfg = Qwen2_5OmniThinkerConfig(text_config=text, vision_config=dict(depth=1, out_hidden_size=D),
                                   audio_config=dict(encoder_layers=1, output_dim=D), image_token_index=VOCAB - 1,
                                   video_token_index=VIDEO_ID, audio_token_index=AUDIO_ID, audio_start_token_id=AS,
                                   audio_end_token_id=AE, position_id_per_seconds=PPS, seconds_per_chunk=CHUNK)
    cfg.vision_start_token_id, cfg.vision_end_token_id = VS, VE
    cfg._attn_implementation = "sdpa"
    with torch.device(dev):
        model = Qwen2_5OmniThinkerForConditionalGeneration(cfg)
    return model.to(torch.bfloat16).eval()


def prompt(dev):
    n_audio = ((N_FEAT - 1) // 2 + 1 - 2) // 2 + 1
    per_chunk = PPS * CHUNK
    parts = [torch.full((40,), TEXT_ID), torch.tensor([VS, AS])]
    for j in range(max(FRAMES // CHUNK, -(-n_audio // per_chunk))):     # v0 a0 v1 a1 ... (2 frames, 50 audio tokens)
        if j < FRAMES // CHUNK:
            parts.append(torch.full((CHUNK * PER_FRAME,), VIDEO_ID))
        a = min(per_chunk, n_audio - j * per_chunk)
        if a > 0:
            parts.append(torch.full((a,), AUDIO_ID))
    parts += [torch.tensor([AE, VE]), torch.full((30,), TEXT_ID)]
    ids = torch.cat(parts)[None].to(dev)
    video = synth.make(FRAMES, PER_FRAME, D, torch.bfloat16, 7, "drift").reshape(FRAMES * PER_FRAME, D).to(dev)
    audio = synth.to_torch(synth.gauss(8, 45, 0, n_audio * D).reshape(n_audio, D), torch.bfloat16).to(dev)
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), use_audio_in_video=True, use_cache=True,
              pixel_values_videos=torch.zeros(1, 4, device=dev),
              video_grid_thw=torch.tensor([[FRAMES, HW, HW]], device=dev),
              video_second_per_grid=torch.ones(1, device=dev),
              input_features=torch.zeros(1, 128, N_FEAT, device=dev),
              feature_attention_mask=torch.ones(1, N_FEAT, dtype=torch.int64, device=dev))
    return kw, video, audio


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.25)
    args = ap.parse_args()
    os.environ["COMPRESSOR"], os.environ["R_RATIO"] = "vidcom2", str(args.ratio)
    dev = "cuda"
    model = thinker(args.layers, dev)
    kw, video, audio = prompt(dev)
    model.__dict__["get_video_features"] = lambda *a, **k: SimpleNamespace(pooler_output=(video,))
    model.__dict__["get_audio_features"] = lambda *a, **k: SimpleNamespace(last_hidden_state=audio)
    with torch.no_grad():
        plain = timed(lambda: model(**kw), args.steps, args.warmup)
        model.forward = types.MethodType(Qwen2_5OmniThinker_forward, model)
        hooked = timed(lambda: model(**kw), args.steps, args.warmup)
    st = model._vidcom2_last
    print(json.dumps(dict(workload=f"Qwen2.5-Omni thinker, D={D}, {args.layers} layers, {FRAMES}x{PER_FRAME} video "
                                   f"tokens + {audio.shape[0]} interleaved audio tokens, bf16, R_RATIO={args.ratio}",
                          S=int(kw["input_ids"].shape[1]), S_pruned=int(st.keep_token_indices.numel()),
                          pruned=bool(st.pruned), unhooked_ms=round(plain, 3), hooked_ms=round(hooked, 3),
                          speedup=round(plain / hooked, 3))))


if __name__ == "__main__":
    main()

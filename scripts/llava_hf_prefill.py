#!/usr/bin/env python
"""One LLaVA-OneVision prefill through transformers' `LlavaOnevisionForConditionalGeneration`: unhooked against hooked
(video tokens pruned) against hooked with `VC2_FUSED_POOL=on`.  Random weights at LLaVA-OneVision-7B text width
(D = 3584, Qwen2-7B's MLP width and heads) with few decoder layers and a small vocabulary; one 32-frame video (27x27
projected patches per frame, pooled to 196 tokens), bf16.  The vision tower and the projector are bypassed -- the video
enters as synthetic projector output -- but the model's `apply_pooling` runs, so the times are pooling + the pruning
step + the decoder stack and lm_head.  The three variants alternate in one process (same model, same inputs), every
time a hipEvent pair around one forward; the medians over all rounds are printed as one JSON line and appended to
`--out`:

  unhooked_ms / hooked_ms / hooked_fused_pool_ms   prefill (use_cache=True); *_minmax: the spread over the rounds
  S / S_pruned                                     prompt length before / after pruning

    python scripts/llava_hf_prefill.py [--layers 4] [--frames 32] [--rounds 10] [--warmup 3] [--ratio 0.25]
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vidcom2_amd import synth                                                   # noqa: E402
from vidcom2_amd.models import install                                          # noqa: E402

D, SIDE, VOCAB, TEXT_ID, IMAGE_ID, VIDEO_ID = 3584, 27, 8192, 100, 8000, 8001
PER_FRAME = ((SIDE + 1) // 2) ** 2


def build(layers, dev):
    from transformers.models.llava_onevision import LlavaOnevisionConfig
    from transformers.models.llava_onevision.modeling_llava_onevision import LlavaOnevisionForConditionalGeneration
    text = dict(model_type="qwen2", vocab_size=VOCAB, hidden_size=D, intermediate_size=18944, num_hidden_layers=layers,
                num_attention_heads=28, num_key_value_heads=4, max_position_embeddings=32768)
    vision = dict(model_type="siglip_vision_model", hidden_size=32, intermediate_size=32, num_hidden_layers=1,
                  num_attention_heads=2, image_size=SIDE * 14, patch_size=14, vision_use_head=False)
    cfg = LlavaOnevisionConfig(vision_config=vision, text_config=text, image_token_id=IMAGE_ID, video_token_id=VIDEO_ID,
                               vision_feature_layer=-1, vision_feature_select_strategy="full", tie_word_embeddings=False)
    cfg._attn_implementation = "sdpa"
    with torch.device(dev):
        model = LlavaOnevisionForConditionalGeneration(cfg)
    return model.to(torch.bfloat16).eval()


def inputs(frames, dev):
    ids = torch.cat((torch.full((40,), TEXT_ID), torch.full((frames * PER_FRAME + 1,), VIDEO_ID),
                     torch.full((30,), TEXT_ID)))[None].to(dev)
    projected = synth.make(frames, SIDE * SIDE, D, torch.bfloat16, 7, "drift").reshape(frames, SIDE * SIDE, D).to(dev)
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), use_cache=True,
              pixel_values_videos=torch.zeros(1, frames, 3, 1, 1, dtype=torch.bfloat16, device=dev))
    return kw, projected


def bypass_tower(inner, projected):
    """`get_video_features` stays the model's own; its tower and projector hand it the synthetic projector output."""
    inner.__dict__["vision_tower"] = lambda *a, **k: SimpleNamespace(hidden_states=(projected,))
    inner.__dict__["multi_modal_projector"] = lambda x: x


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "llava_hf_prefill.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("llava_hf_prefill.py measures on a ROCm GPU; none found")
    os.environ["COMPRESSOR"], os.environ["R_RATIO"] = "vidcom2", str(args.ratio)
    os.environ.pop("VC2_BATCHED_PREFILL", None)
    dev = "cuda"
    model = build(args.layers, dev)
    kw, projected = inputs(args.frames, dev)
    bypass_tower(model.model, projected)
    assert install(model)
    bound = {m: m.__dict__["forward"] for m in (model, model.model)}

    def run_plain():
        # the same model without the hook: the bound hooks leave the two instances for the length of this call
        for m in bound:
            del m.__dict__["forward"]
        try:
            model(**kw)
        finally:
            for m, hook in bound.items():
                m.__dict__["forward"] = hook

    def run_hooked(knob):
        def run():
            os.environ["VC2_FUSED_POOL"] = knob
            model(**kw)
        return run

    variants = dict(unhooked=run_plain, hooked=run_hooked("off"), hooked_fused_pool=run_hooked("on"))
    times = {k: [] for k in variants}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        for _ in range(args.rounds):                # alternating: a drift of the machine hits every variant alike
            for name, fn in variants.items():
                times[name].append(once(fn))
        run_hooked("off")()
        st = model.model._vidcom2_last
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = dict(workload=f"LlavaOnevisionForConditionalGeneration, D={D}, {args.layers} layers, {args.frames}x{SIDE}x{SIDE}"
                         f" projected patches -> {args.frames}x{PER_FRAME} video tokens + newline, bf16, "
                         f"R_RATIO={args.ratio}, towers bypassed, apply_pooling included",
                S=int(kw["input_ids"].shape[1]), S_pruned=int(st.keep_token_indices.numel()), pruned=bool(st.pruned),
                rounds=args.rounds, device=torch.cuda.get_device_name(0))
    for k, v in times.items():
        line[f"{k}_ms"] = round(med[k], 3)
        line[f"{k}_minmax"] = [round(min(v), 3), round(max(v), 3)]
    line["speedup_hooked"] = round(med["unhooked"] / med["hooked"], 3)
    line["speedup_hooked_fused_pool"] = round(med["unhooked"] / med["hooked_fused_pool"], 3)
    print(json.dumps(line))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

"""Time and size the chunked pass (`compress_chunks`, vidcom2_amd/chunked.py) against concatenating the chunks first.

Shapes: cfg4 (512 x 196 x 3584 bf16 in 8 chunks of 64 frames) and the target shape (128 frames in 4 chunks of 32), retain
0.25, `synth` inputs ("drift").  One process; the legs alternate inside every round.  A leg's figure is the host time of one
call that ends in the pass's own device synchronise (all three legs return after their single host read):
    chunks       (a) compress_chunks(chunks)
    cat          (b) compress(torch.cat(chunks))  -- what a caller has to do without the chunked pass
    contiguous   (c) compress(x) on a tensor that is contiguous already
A round's figure is the median of `--iters` calls after `--warmup`; a leg's record holds the median of the round medians
and their range (the run-to-run spread).  Peak memory: torch.cuda.max_memory_allocated above the bytes allocated with
the chunks resident, for (a) and (b), each from cold caches (no cached plan or compressor).  Where (a)'s time goes: the
library's per-kernel timing (vc2_profile_collect) over a few passes of (a) and (c), in passes of their own (the timing
brackets every launch with events).  The three legs must agree bit for bit before their times are compared.
LLaVA-Video's shape (128 x 169 x 3584 bf16 in 4 chunks of 32 frames, the 13 x 13 grid with the newline vector) has two legs
of its own, time and peak memory above the resident inputs each:
    llava_vid         compress_chunks(chunks, 169, mapper="grid_vid", grid_h=13, newline=) against
                      compress(torch.cat(chunks), 169, "grid_vid", 13, newline=)
    llava_vid_pooled  the chunks as the projector's [32, 26 * 26, 3584] output: ChunkedCompressor.add_pooled per chunk against
                      fused.pool_stats per chunk + add (the same compressor options)
Writes one JSON line per shape to profiles/chunked_bench.jsonl.

The run ends itself after `--time-limit` seconds (default 900) with exit status 124.

    python scripts/chunked_bench.py [--rounds 3] [--iters 20] [--warmup 5]
                                    [--shapes cfg4,target,llava_vid,llava_vid_pooled] [--out FILE]
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import signal
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import vidcom2_amd as vc  # noqa: E402
from vidcom2_amd import _ffi, chunked, fused, synth  # noqa: E402
from vidcom2_amd.vidcom2 import clear_plan_cache  # noqa: E402

SHAPES = {"cfg4": (512, 196, 3584, torch.bfloat16, [64] * 8), "target": (128, 196, 3584, torch.bfloat16, [32] * 4)}
VID = (128, 169, 3584, torch.bfloat16, [32] * 4, 13)       # LLaVA-Video: 13 x 13 tokens per frame, pooled from 26 x 26
BASE = 0.25
LEGS = ("chunks", "cat", "contiguous")


def timed(fn, iters, warmup):
    """Median microseconds of fn(), a call that returns after its own device synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    return statistics.median(ts)


def summary(vals):
    return {"median_us": round(statistics.median(vals), 1), "min_us": round(min(vals), 1), "max_us": round(max(vals), 1),
            "rounds": [round(v, 1) for v in vals]}


def peak_above(fn):
    """Peak bytes allocated during fn() above what is allocated now, from cold caches."""
    clear_plan_cache()
    chunked.clear_chunk_cache()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def kernels(fn, n=5):
    """{kernel: {us_per_pass, launches_per_pass}} over n passes, from vc2_profile_collect."""
    fn()
    torch.cuda.synchronize()
    _ffi.profile_enable(True)
    try:
        before = _ffi.profile_collect()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        after = _ffi.profile_collect()
    finally:
        _ffi.profile_enable(False)
    out = {}
    for k, (ms, cnt) in after.items():
        ms0, cnt0 = before.get(k, (0.0, 0))
        if cnt - cnt0:
            out[k] = {"us_per_pass": round((ms - ms0) * 1e3 / n, 1), "launches_per_pass": round((cnt - cnt0) / n, 1)}
    out["sum_us_per_pass"] = round(sum(v["us_per_pass"] for v in out.values()), 1)
    return out


def one_shape(name, args):
    F, N, D, dtype, frames = SHAPES[name]
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, dtype, 0, "drift").to(dev)
    chunks, f0 = [], 0
    for f in frames:
        chunks.append(x[f0 * N: (f0 + f) * N].clone())
        f0 += f
    _ffi.set_mode("torch")
    legs = {"chunks": lambda: vc.compress_chunks(chunks, N, BASE), "cat": lambda: vc.compress(torch.cat(chunks), N, BASE),
            "contiguous": lambda: vc.compress(x, N, BASE)}
    a, b, c = (legs[k]() for k in LEGS)
    it = torch.int16
    same = all(r.K == c.K and bool(torch.equal(r.global_idx, c.global_idx)) and bool(torch.equal(r.ks, c.ks))
               and bool(torch.equal(r.rows.view(it), c.rows.view(it))) for r in (a, b))
    K = int(c.K)
    del a, b, c
    rounds = {k: [] for k in LEGS}
    for _ in range(args.rounds):
        for k in LEGS:
            rounds[k].append(timed(legs[k], args.iters, args.warmup))
    video = F * N * D * x.element_size()
    rec = {"shape": name, "F": F, "N": N, "D": D, "dtype": str(dtype).replace("torch.", ""), "chunks": frames, "base": BASE,
           "dist": "drift", "seed": 0, "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup, "K": K,
           "legs_bit_identical": same, "video_bytes": video, "legs": {k: summary(v) for k, v in rounds.items()}}
    L = rec["legs"]
    rec["chunks_minus_cat_us"] = round(L["chunks"]["median_us"] - L["cat"]["median_us"], 1)
    rec["chunks_minus_contiguous_us"] = round(L["chunks"]["median_us"] - L["contiguous"]["median_us"], 1)
    rec["kernels_chunks"] = kernels(legs["chunks"])
    rec["kernels_contiguous"] = kernels(legs["contiguous"])
    del x                                                   # (the chunks alone are resident for the memory figures)
    legs.pop("contiguous")
    rec["peak_bytes_above_chunks"] = {"chunks": peak_above(legs["chunks"]), "cat": peak_above(legs["cat"])}
    return rec


def two_legs(name, args, legs, extra, cold=lambda: None):
    """Two legs that must agree bit for bit: alternating timed rounds, then each one's peak memory from cold caches
    (cold() drops what the legs themselves keep between calls)."""
    (ka, a), (kb, b) = ((k, fn()) for k, fn in legs.items())
    it = torch.int16
    same = a.K == b.K and bool(torch.equal(a.global_idx, b.global_idx)) and bool(torch.equal(a.ks, b.ks)) \
        and bool(torch.equal(a.rows.view(it), b.rows.view(it)))
    K = int(a.K)
    del a, b
    rounds = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k in legs:
            rounds[k].append(timed(legs[k], args.iters, args.warmup))
    F, N, D, dtype, frames, h = VID
    rec = {"shape": name, "F": F, "N": N, "D": D, "dtype": str(dtype).replace("torch.", ""), "chunks": frames, "grid_h": h,
           "base": BASE, "dist": "drift", "seed": 0, "rounds": args.rounds, "iters": args.iters, "warmup": args.warmup, "K": K,
           "legs_bit_identical": same, "legs": {k: summary(v) for k, v in rounds.items()}}
    rec.update(extra)
    rec[f"{ka}_minus_{kb}_us"] = round(rec["legs"][ka]["median_us"] - rec["legs"][kb]["median_us"], 1)
    rec["peak_bytes_above_inputs"] = {}
    for k, fn in legs.items():
        cold()
        rec["peak_bytes_above_inputs"][k] = peak_above(fn)
    return rec


def llava_vid(name, args):
    F, N, D, dtype, frames, h = VID
    dev = torch.device("cuda:0")
    _ffi.set_mode("torch")
    nl = torch.randn(D, generator=torch.Generator().manual_seed(1)).to(dtype).to(dev)
    if name == "llava_vid":
        x = synth.make(F, N, D, dtype, 0, "drift").to(dev)
        chunks = list(x.split([f * N for f in frames]))
        chunks = [c.clone() for c in chunks]
        del x
        legs = {"chunks": lambda: vc.compress_chunks(chunks, N, BASE, mapper="grid_vid", grid_h=h, newline=nl),
                "cat": lambda: vc.compress(torch.cat(chunks), N, BASE, "grid_vid", h, newline=nl)}
        return two_legs(name, args, legs, {"video_bytes": F * N * D * 2})
    # the projector's output per chunk, [F_c, 26 * 26, D]; both legs run one compressor object of their own
    H = 2 * h
    imgs = [synth.make(f, H * H, D, dtype, 10 + c, "drift").to(dev).view(f, H * H, D) for c, f in enumerate(frames)]
    ccs = {}

    def compressor(k):
        if k not in ccs:
            ccs[k] = vc.ChunkedCompressor(frames, N, D, dtype, dev, BASE, mapper="grid_vid", grid_h=h, newline=nl)
        return ccs[k]

    def pooled():
        cc = compressor("add_pooled")
        for x in imgs:
            cc.add_pooled(x, H, H, "average")
        return cc.finish()

    def pool_then_add():
        cc = compressor("pool_add")
        for x in imgs:
            cc.add(fused.pool_stats(x, H, H, "average")[0].view(-1, D))
        return cc.finish()
    return two_legs(name, args, {"add_pooled": pooled, "pool_add": pool_then_add},
                    {"pool": "average", "input_bytes": F * H * H * D * 2, "video_bytes": F * N * D * 2}, cold=ccs.clear)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="cfg4,target,llava_vid,llava_vid_pooled")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunked_bench.jsonl"))
    ap.add_argument("--time-limit", type=int, default=900, help="seconds after which the run ends itself")
    args = ap.parse_args()

    def out_of_time(*_):
        print(f"[chunked_bench] time limit of {args.time_limit} s reached", flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, out_of_time)
    signal.alarm(args.time_limit)
    if args.iters < 20 or args.warmup < 5:
        raise SystemExit("chunked_bench: at least 20 timed calls after at least 5 warm-ups per round")
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    head = {"script": "scripts/chunked_bench.py", "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for name in args.shapes.split(","):
            rec = dict(head, **(one_shape(name, args) if name in SHAPES else llava_vid(name, args)))
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")
            chunked.clear_chunk_cache()
            clear_plan_cache()
            gc.collect()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

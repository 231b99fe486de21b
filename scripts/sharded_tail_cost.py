"""What the wide exchange-2b records (the C % 32 tail replay of the frame-sharded pass) cost on the GPU: the summed time
of one rank's record + finish kernels (`k_vc_records` in vc2_profile_collect) for two emulated ranks of 64 x 196 x 3584
fp16 frames each, at ratio 0.25 (C = 896: empty tail, narrow records), at ratio 0.3 (C = 1075: 19 tail columns, wide
records) in the default mode and at ratio 0.3 in `torch_proven`.  Three repetitions each -> one JSON line per leg.

    python scripts/sharded_tail_cost.py [out.jsonl]
"""
import json
import sys

import torch

from vidcom2_amd import PassParams, _ffi, synth
from vidcom2_amd.sharded import HipStages


def one_pass(st, shards, f0s, F, N, timed):
    """The stage chain of both ranks; the profile is switched on only around rank `timed`'s exchange-2b calls."""
    stats_all = torch.stack([s.chan_stats(x).clone() for s, x in zip(st, shards)])
    for s in st:
        s.select_channels(stats_all, F * N)
    csum_all = torch.stack([s.phase1(x).clone() for s, x in zip(st, shards)])

    def on(p):
        torch.cuda.synchronize()
        _ffi.profile_enable(p == timed)

    blocks = []
    for p, (s, x, f0) in enumerate(zip(st, shards, f0s)):
        on(p)
        blocks.append(s.vc_blocks(x, csum_all, F * N, f0))
    on(-1)
    flagged = st[0].flagged_columns()
    if st[0].needs_rounds():
        for j0 in range(0, max(flagged, 1), st[0].vc_cap):
            if j0:
                blocks = []
                for p, (s, x, f0) in enumerate(zip(st, shards, f0s)):
                    on(p)
                    blocks.append(s.vc_blocks_round(x, F * N, f0, j0))
                on(-1)
            blocks_all = torch.stack([b.clone() for b in blocks])
            for p, s in enumerate(st):
                on(p)
                s.vc_finish_round(F * N, blocks_all, j0)
            on(-1)
        for s, x in zip(st, shards):
            s.phase2(x, csum_all, F * N, vc_final=True)
    else:
        blocks_all = torch.stack([b.clone() for b in blocks])
        for p, (s, x) in enumerate(zip(st, shards)):
            on(p)
            s.phase2(x, csum_all, F * N, blocks_all)
        on(-1)
    torch.cuda.synchronize()
    return flagged


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else "profiles/sharded_tail_records.jsonl"
    Fl, N, D, W = 64, 196, 3584, 2
    F = Fl * W
    dev = torch.device("cuda:0")
    x = synth.make(F, N, D, torch.float16, 1, "drift").to(dev)
    shards = [x[p * Fl * N: (p + 1) * Fl * N].contiguous() for p in range(W)]
    f0s = [p * Fl for p in range(W)]
    lines = []
    for ratio, mode in ((0.25, "torch"), (0.3, "torch"), (0.3, "torch_proven")):
        _ffi.set_mode(mode)
        try:
            st = [HipStages(Fl, N, D, torch.float16, dev, 0.25, params=PassParams(ratio)) for _ in range(W)]
            for s in st:
                s.F_total = F
            one_pass(st, shards, f0s, F, N, timed=-1)                       # warm-up
            reps = []
            for _ in range(3):
                _ffi.profile_enable(False)
                _ffi.profile_collect()
                flagged = one_pass(st, shards, f0s, F, N, timed=0)
                got = _ffi.profile_collect().get("k_vc_records", (0.0, 0))
                reps.append({"us": round(got[0] * 1e3, 1), "launches": got[1]})
            lines.append({"shape": [Fl, N, D], "ranks": W, "dtype": "f16", "ratio": ratio, "C": st[0].C, "mode": mode,
                          "tail_columns": st[0].C % 32, "wide_records": bool(st[0].vc_tail), "flagged": flagged,
                          "record_floats": int(st[0].blocks.shape[1]), "k_vc_records": reps,
                          "fragile": [int(s.kout[2]) for s in st]})
        finally:
            _ffi.set_mode("torch")
            _ffi.profile_enable(False)
    with open(out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
            print(json.dumps(ln))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""The drain behind sweeps 1 and 2 (NOTES_r07.md, Step 0): last stamp of the sweep's last workgroup against the first stamp
of the launch that reads its partials (k_var_select's variance workgroups, k_frame_centres' frame workgroups), and which
workgroups of k_dist / sweep 2 share a CU (hardware id next to the stamps).
Library built with -DVC2_DEBUG_TIMING:  python scripts/dev/s0_drain.py lib.so [passes]"""
import ctypes, os, sys
os.environ["VC2_LIB_PATH"] = os.path.abspath(sys.argv[1])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
F, N, D = 128, 196, 3584
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 6
x = synth.make(F, N, D, torch.bfloat16, 0, "drift").cuda()
plan = vc.vidcom2.CompressPlan(F, N, D, torch.bfloat16, x.device, 0.25)
L = ctypes.CDLL(_ffi.LIB_PATH)
wg = (ctypes.c_ulonglong * (8 * 2 * 4096))()
s0 = (ctypes.c_ulonglong * (8 * 4096))()
rows = []
for it in range(passes):
    plan.enqueue(x); plan.finish()
    torch.cuda.synchronize()
    L.vc2_debug_wg(wg); L.vc2_debug_s0(s0)
    a = np.frombuffer(wg, dtype=np.uint64).reshape(8, 2, 4096).astype(np.float64) / 100.0
    s = np.frombuffer(s0, dtype=np.uint64).reshape(8, 4096).copy()
    t = s[:4].astype(np.float64) / 100.0
    nz = lambda v: v[v > 0]
    b1, e1, v0, c0 = nz(t[0]), nz(t[1]), nz(t[2]), nz(t[3])
    e2, loop2 = nz(a[1, 1]), nz(a[4, 1])
    rows.append((e1.max() - b1.min(), np.percentile(e1 - b1.min(), 50), v0.min() - e1.max(),
                 loop2.max() - nz(a[1, 0]).min(), e2.max() - nz(a[1, 0]).min(), c0.min() - e2.max()))
print("pass | k_chan_stats: last end, median end, gap to k_var_select's first variance workgroup | "
      "sweep 2: last row loop end, last end, gap to k_frame_centres' first frame workgroup  (us; pass 0 is cold)")
for i, r in enumerate(rows):
    print(f"{i:4d} | {r[0]:6.2f} {r[1]:6.2f} {r[2]:6.2f} | {r[3]:6.2f} {r[4]:6.2f} {r[5]:6.2f}")
m = np.median(np.array(rows[1:]), axis=0)
print("median of the warm passes:", " ".join(f"{v:.2f}" for v in m),
      f"| drain beyond the 1.5 us plain boundary: sweep 1 {m[2] - 1.5:+.2f}, sweep 2 {m[5] - 1.5:+.2f} us")
# who shares a CU: key = (XCC id, SE / SH / CU id bits 8..15 of HW_ID)
for slot, name, n in ((4, "k_dist", F * 8), (5, "sweep 2", 512)):
    h = s[slot][:n]
    ids = np.where(h != 0)[0]
    key = ((h[ids] >> np.uint64(32)) << np.uint64(8)) | ((h[ids] >> np.uint64(8)) & np.uint64(0xFF))
    cus = {}
    for i, k in zip(ids.tolist(), key.tolist()):
        cus.setdefault(k, []).append(i)
    sizes = np.bincount([len(v) for v in cus.values()])
    print(f"{name}: {len(ids)} workgroups on {len(cus)} CUs; CUs by workgroups held:", {i: int(c) for i, c in enumerate(sizes) if c})
    if slot == 4:
        pat = {}
        for v in cus.values():
            p = tuple(sorted(i // F for i in v))
            pat[p] = pat.get(p, 0) + 1
        print("   splits (blockIdx / F) sharing a CU, most common:", sorted(pat.items(), key=lambda kv: -kv[1])[:6])
        lv = lambda f_: sum(1 for v in cus.values() if len({f_(i // F) for i in v}) == len(v))
        print(f"   CUs whose workgroups all get different levels: sp >> 1: {lv(lambda sp: sp >> 1)}, sp & 3: {lv(lambda sp: sp & 3)}, of {len(cus)}")
    else:
        pairs = sum(1 for v in cus.values() if len(v) == 2 and abs(v[0] - v[1]) == 256)
        print(f"   CUs holding exactly the pair (i, i + 256): {pairs}; CUs holding two workgroups >= 256: "
              f"{sum(1 for v in cus.values() if sum(i >= 256 for i in v) >= 2)}")

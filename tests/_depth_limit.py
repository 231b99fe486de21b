"""Loader of tests/golden/depth_limit_kat.npz (make_depth_limit_golden.py): inputs that drive torch.topk's nth_element /
sort into libstdc++'s depth-limit fall-backs, stored as value ranks plus the rule that turns a rank into a value."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DTYPES = ("bf16", "f16", "f32")
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
# value of rank r = the bit pattern START + r: positive finite 16-bit values (exactly representable: 32-bit selection words),
# or fp32 values one ulp apart above 1.0 (not 16-bit representable: 64-bit selection words)
START = {"bf16": 0x3000, "f16": 0x0400, "f32": 0x3F800001}
# amplitudes of the fused-pass inputs: every SECOND 16-bit value, the range centred on 1.0
ONE = {"bf16": 0x3F80, "f16": 0x3C00}


def _from_bits(bits, dn):
    if dn == "f32":
        return torch.from_numpy(bits.astype(np.int32)).view(torch.float32)
    return torch.from_numpy(bits.astype(np.int16)).view(TORCH_DT[dn])


def rank_values(ranks, dn):
    """The fixture's values in dtype dn (a 1-D CPU tensor)."""
    return _from_bits(np.asarray(ranks).astype(np.int64) + START[dn], dn)


def amp_values(ranks, dn):
    r = np.asarray(ranks).astype(np.int64)
    return _from_bits(ONE[dn] - (int(r.max()) + 1) + 2 * r, dn)


def pass_input(ranks, F, N, dn, seed=7):
    """x [F*N, D]: column c is a balanced +-1 pattern (its own) times amplitude c, so var(x, 0)[c] = RN(amplitude^2): the
    variances carry the rank pattern, its order and its ties."""
    R, D = F * N, len(ranks)
    assert R % 2 == 0
    sign = (np.random.RandomState(seed).rand(R, D).argsort(0) % 2).astype(np.float32) * 2.0 - 1.0
    return (torch.from_numpy(sign) * amp_values(ranks, dn).float()[None, :]).to(TORCH_DT[dn])


def load():
    """-> list of dicts: name, kind (0 select, 1 sort, 2 fused-pass amplitudes), n, k, sorted, ranks, out, and the certificate
    (sel_hit, sel_len, sel_pops = elements the fall-back's __heap_select took in, group, group_kept, naive_differs, flip_differs
    = a heap step that breaks ties the other way changes the kept set, segs [(first, last)], seg_dup, disorder; pass: F, N,
    dtype)."""
    z = np.load(os.path.join(GOLDEN, "depth_limit_kat.npz"))
    assert z["start"].tolist() == [START[d] for d in DTYPES]
    out, npass = [], 0
    for i in range(len(z["k"])):
        s0, s1 = int(z["seg_off"][i]), int(z["seg_off"][i + 1])
        c = dict(name=str(z["names"][i]), kind=int(z["kind"][i]), n=int(z["n"][i]), k=int(z["k"][i]), sorted=bool(z["sorted"][i]),
                 ranks=z["ranks"][z["offs_v"][i]: z["offs_v"][i + 1]],
                 out=z["out"][z["offs_o"][i]: z["offs_o"][i + 1]].astype(np.int64),
                 sel_hit=bool(z["sel_hit"][i]), sel_len=int(z["sel_len"][i]), group=int(z["group"][i]),
                 group_kept=int(z["group_kept"][i]), naive_differs=bool(z["naive_differs"][i]),
                 segs=[tuple(int(v) for v in sg) for sg in z["seg"][s0:s1]], seg_dup=[bool(d) for d in z["seg_dup"][s0:s1]],
                 disorder=bool(z["disorder"][i]), sel_pops=int(z["sel_pops"][i]), flip_differs=bool(z["flip_differs"][i]))
        if c["kind"] == 2:
            F, N, D, dti = (int(v) for v in z["pass_shape"][npass])
            assert D == c["n"]
            c.update(F=F, N=N, dtype=DTYPES[dti])
            npass += 1
        out.append(c)
    return out

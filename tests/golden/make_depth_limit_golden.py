#!/usr/bin/env python3
"""Fixtures that drive torch.topk(largest=False) into libstdc++'s depth-limit fall-backs, with ties.

    python tests/golden/make_depth_limit_golden.py        ->  tests/golden/depth_limit_kat.npz

torch.topk on the CPU is std::nth_element (+ std::sort of the first k-1 when sorted=True) on (value, index) pairs
(ATen/native/TopKImpl.h; oracle/vc2_oracle.cpp topk_smallest).  Both give up on quicksort after 2*floor(log2 n)
partitions: __introselect finishes with __heap_select(first, nth + 1, last); iter_swap(first, nth), __introsort_loop
heap-sorts the segment it is on.  Random inputs never get there, so the device replay of those branches
(vidcom2_amd/csrc/vc2_select2.h) needs inputs built for it.  Two adversaries build them; their victim is the real
std:: code of this machine's libstdc++ (depth_limit_adversary.cpp, compiled here with g++ into a temporary directory).

Selection: McIlroy's "antiquicksort" (A Killer Adversary for Quicksort, 1999).  The comparator is lazy: every value starts
as "gas", larger than anything solid; when two gas values meet, the one that was the last to be compared against something
solid -- the pivot candidate -- is frozen to the next smallest solid value.  Every partition then peels off a pivot and
one or two more elements, and nth_element meets its depth limit with nearly the whole array still open.  The adversary
runs on the identity arrangement, so the frozen values ARE the input; replayed through the real nth_element the concrete
values make exactly the comparisons of the adversarial run (asserted below).  Left at that, the fall-back has nothing to
decide: the lazy values arrive in an order in which __heap_select never takes an element into its heap after __make_heap,
so the kept set is what the partitions left in front and a replay that skipped the fall-back would still return it.  So
when the limit is met, every value that is still gas gets its place in a seeded random order instead (gas has only been
called larger than something solid, so any values above the solid ones keep all answers given so far): the partitions
are McIlroy's, the __heap_select has a third of the range to take in.  (That adversary runs against the transcription
below, which knows where the limit is; the fixture is then certified against the real std:: calls like every other.)

Sort: the same adversary cannot go on through the std::sort that follows, because nth_element has frozen every kept value
by then.  So two phases.  In phase 1 nth_element is answered from a fixed random permutation sigma while the comparator
records who met whom.  An element that only ever met hubs (elements with at least 17 partners: the pivots) is not pinned
any further than "between the two hubs around it": it becomes gas again, above every solid of that sigma interval and below
the hub that closes it -- all phase-1 answers stay what they were.  In phase 2 std::sort is answered with McIlroy's rule
among the gas of one interval.  The sort then meets depth 0 on a long segment of such an interval.

Ties: with distinct values the kept set and the sorted order are unique and ANY correct fall-back passes; what the replay
must get right is the permutation of equal values.  Adjacent ranks are therefore tied IN PAIRS (value = (rank + off) // 2):
a pair hardly changes what a partition sees, and every case keeps its depth limit.  Tying in threes or wider does not: the
Hoare partition stops on equal keys from both sides, the partitions become balanced and the limit is never met.  Only at
the selection boundary a slightly wider group is searched for (ranks k-1-a .. k-1+b tied together), because with a
boundary pair the reference's choice is always "lowest index" or "highest index" and a replay with a naive tie rule would
pass.  Among the variants that keep the limit, one wins whose kept set differs from both naive rules AND changes when
__adjust_heap takes the other of two equal children (the transcription's deliberately wrong run): a fixture that no slip
can change checks nothing.

Every fixture is certified by an instrumented transcription of __introselect / __introsort_loop (same file) run on the
concrete values: it must give the permutation of the real std:: calls, and it reports whether the selection met its
limit (and with which range) and which sort segments were heap-sorted.  The generator refuses to write a fixture that
misses its conditions (see check_select / sort_conditions / pass_case).

Values are stored as value ranks (uint16) plus a rule: the r-th value above a stated start bit pattern -- positive finite
bf16 / fp16 values for the 16-bit cases (exactly representable: the 32-bit word engines run), fp32 values one ulp apart
for the fp32 cases (not 16-bit representable: the 64-bit word engines run).  Expected outputs are torch.topk's, per dtype.

The second half builds inputs for the FUSED pass: x [F*N, D] whose channel variances carry a killer rank pattern (a balanced
+-1 column pattern times a per-channel amplitude, every second representable 16-bit value, so that the rounded variances
stay distinct where the pattern is distinct and equal where it is tied).  Only the amplitude ranks are stored.
"""
from __future__ import annotations

import ctypes
import io
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from _depth_limit import DTYPES, START, pass_input, rank_values  # noqa: E402

MAXSEG = 64
HUB_MIN = 17

_helper = None


def helper():
    """depth_limit_adversary.cpp as a shared library in a temporary directory."""
    global _helper
    if _helper is None:
        d = tempfile.mkdtemp(prefix="depth_limit_")
        so = os.path.join(d, "libdepthlimit.so")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so,
                               os.path.join(HERE, "depth_limit_adversary.cpp")])
        L = ctypes.CDLL(so)
        for f in (L.dl_real, L.dl_trace, L.dl_antiqs_select, L.dl_antiqs_select_busy, L.dl_antiqs_sort):
            f.restype = ctypes.c_long
        _helper = L
    return _helper


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def real(v, k, srt):
    perm = np.empty(v.size, np.int64)
    ncmp = helper().dl_real(_ptr(v), int(v.size), int(k), int(srt), _ptr(perm))
    return perm, ncmp


def trace(v, k, srt, flip=0):
    """-> (perm, certificate dict) from the instrumented transcription (flip: with the deliberately wrong heap step)."""
    perm = np.empty(v.size, np.int64)
    cert = np.zeros(5, np.int32)
    sf, sl = np.zeros(MAXSEG, np.int32), np.zeros(MAXSEG, np.int32)
    ncmp = helper().dl_trace(_ptr(v), int(v.size), int(k), int(srt), _ptr(perm), _ptr(cert), _ptr(sf), _ptr(sl), MAXSEG, int(flip))
    ns = int(cert[3])
    assert ns <= MAXSEG
    return perm, {"hit": int(cert[0]), "len": int(cert[1]), "parts": int(cert[2]), "pops": int(cert[4]), "ncmp": int(ncmp),
                  "segs": [(int(sf[i]), int(sl[i])) for i in range(ns)]}


def antiqs_select(n, k):
    rank = np.empty(n, np.int32)
    ncmp = helper().dl_antiqs_select(n, k, _ptr(rank))
    return rank, ncmp


def antiqs_select_busy(n, k, seed):
    rank = np.empty(n, np.int32)
    ncmp = helper().dl_antiqs_select_busy(n, k, ctypes.c_uint(seed), _ptr(rank))
    return rank, ncmp


def antiqs_sort(n, k, seed):
    sigma = np.random.RandomState(seed).permutation(n).astype(np.int32)
    rank = np.empty(n, np.int32)
    nfree = ctypes.c_int32(0)
    ncmp = helper().dl_antiqs_sort(n, k, _ptr(sigma), HUB_MIN, _ptr(rank), ctypes.byref(nfree))
    return rank, ncmp, int(nfree.value)


def f32_of(ranks):
    """The fp32 values of the bf16 rule (order and ties are those of every rule: all are strictly increasing in the rank)."""
    return rank_values(ranks, "bf16").float().numpy()


def certified(ranks, k, srt):
    """Transcription == real std:: calls (whole permutation, comparison count); -> (perm, certificate)."""
    v = f32_of(ranks)
    p_real, c_real = real(v, k, srt)
    p_tr, cert = trace(v, k, srt)
    assert np.array_equal(p_real, p_tr) and c_real == cert["ncmp"], "the transcription left the real std:: calls"
    return p_real, cert


def boundary(ranks, k, perm):
    """Tie group of the k-th smallest value: (size, kept, differs from lowest-index-first AND highest-index-first)."""
    kth = np.sort(ranks, kind="stable")[k - 1]
    group = np.flatnonzero(ranks == kth)
    kept = np.intersect1d(group, perm[:k])
    m = kept.size
    naive = m > 0 and m < group.size and not np.array_equal(kept, group[:m]) and not np.array_equal(kept, group[group.size - m:])
    return int(group.size), int(m), bool(naive)


def tie(rank, k, off, a=0, b=0):
    """value rank = (rank + off) // 2, with ranks k-1-a .. k-1+b tied together."""
    r = rank.astype(np.int64)
    v = (r + off) // 2
    band = (r >= k - 1 - a) & (r <= k - 1 + b)
    v[band] = (k - 1 + off) // 2
    # dense, order-preserving renumbering
    _, dense = np.unique(v, return_inverse=True)
    return dense.astype(np.uint16)


def second_k(n, k):
    """The next budget above k that round(T(k' / n) * n) gives back in every dtype (a frame's budget is computed in the score
    dtype): the second, different killer of a per-frame shape is the adversary's answer to THAT k."""
    import oracle as O
    from _depth_limit import TORCH_DT
    for k2 in range(k + 1, n):
        if all(O.compute_ks(torch.full((1,), k2 / n, dtype=torch.float32).to(TORCH_DT[d]), n) == [k2] for d in DTYPES):
            return k2
    raise SystemExit(f"no second budget for n={n}")


def flip_differs(ranks, k, perm):
    """Would a heap step that takes the OTHER of two equal children change the kept set?  (dl_trace's deliberately wrong run)"""
    pm, _ = trace(f32_of(ranks), k, False, flip=1)
    return not np.array_equal(np.sort(pm[:k]), np.sort(perm[:k]))


def search_select(n, k, want_hit=True, seed=1):
    """The adversary's ranks, tied: among the tie variants that keep the depth limit and tie the k-th value across the
    boundary, prefer one whose kept set beats both naive tie rules AND changes under a wrong heap step, then the widest group."""
    pure, ncmp_pure = antiqs_select(n, k)
    _, cp = certified(pure.astype(np.uint16), k, False)
    assert cp["ncmp"] == ncmp_pure and bool(cp["hit"]) == want_hit and cp["pops"] == 0      # (McIlroy alone: nothing to select)
    rank, ncmp_adv = antiqs_select_busy(n, k, seed)
    _, c0 = certified(rank.astype(np.uint16), k, False)
    assert c0["ncmp"] == ncmp_adv, "the concrete values do not replay the adversarial run"
    assert bool(c0["hit"]) == want_hit and c0["len"] == cp["len"] and (c0["pops"] > 0) == want_hit, (n, k, c0)
    found = []
    for off in (0, 1):
        for a in range(0, 4):
            for b in range(0, 4):
                r = tie(rank, k, off, a, b)
                perm, cert = certified(r, k, False)
                if bool(cert["hit"]) != want_hit or cert["len"] != c0["len"]:
                    continue
                g, m, naive = boundary(r, k, perm)
                if not (0 < m < g):
                    continue
                flip = flip_differs(r, k, perm)
                found.append(((naive and flip, flip, naive, g, -off), r, cert, (off, a, b)))
    assert found, ("no tie variant keeps the certificate", n, k)
    found.sort(key=lambda t: t[0], reverse=True)
    _, r, cert, var = found[0]
    return r, cert, var


def check_select(name, ranks, k, want_hit):
    perm, cert = certified(ranks, k, False)
    g, m, naive = boundary(ranks, k, perm)
    cert["flip"] = flip_differs(ranks, k, perm)
    if want_hit and cert["pops"] == 0:
        raise SystemExit(f"{name}: the fall-back's __heap_select has nothing to do")
    if bool(cert["hit"]) != want_hit:
        raise SystemExit(f"{name}: depth limit {'not ' if want_hit else ''}met")
    if not (0 < m < g):
        raise SystemExit(f"{name}: the k-th value is not tied across the boundary")
    return perm, cert, g, m, naive


def search_sort(n, k, seeds):
    """Two-phase adversary + pair ties: the first (seed, off) whose certificate holds a heap-sorted segment with duplicates
    that the reference does not leave in index order."""
    for seed in seeds:
        rank, ncmp_adv, nfree = antiqs_sort(n, k, seed)
        _, c0 = certified(rank.astype(np.uint16), k, True)
        assert c0["ncmp"] == ncmp_adv, "the concrete values do not replay the adversarial run"
        if not c0["segs"]:
            continue
        for off in (0, 1):
            r = tie(rank, k, off)
            ok, info = sort_conditions(r, k)
            if ok and info["segs"] == c0["segs"]:
                return r, info, (seed, off, nfree)
    raise SystemExit(f"sort n={n} k={k}: no certified fixture")


def sort_conditions(ranks, k):
    perm, cert = certified(ranks, k, True)
    dup, disorder = [], False
    for (f, l) in cert["segs"]:
        vals, idx = ranks[perm[f:l]], perm[f:l]
        d = bool((vals[1:] == vals[:-1]).any())
        dup.append(d)
        disorder |= bool(((vals[1:] == vals[:-1]) & (idx[1:] < idx[:-1])).any())
    g, m, naive = boundary(ranks, k, perm)
    info = {"segs": cert["segs"], "dup": dup, "disorder": disorder, "hit": cert["hit"], "len": cert["len"], "group": g,
            "kept": m, "naive": naive, "pops": cert["pops"]}
    return bool(cert["segs"]) and any(dup) and disorder, info


# (name, n, k, want the select fall-back, engine class it is for)
SELECT = [
    ("nofb40", 40, 20, False, "frame: one wave, no fall-back (guards the certificate)"),
    ("tail64", 64, 33, True, "frame N<=256 / chan: introselect_tail64 fallback"),
    ("solo196", 196, 49, True, "frame N<=256: topk_smallest4_solo<4> -> introselect_finish"),
    ("chan256", 256, 128, True, "chan D=256: fits one wave at once"),
    ("solo324", 324, 81, True, "frame N<=512: topk_smallest4_solo<8> -> introselect_finish"),
    ("chan512", 512, 256, True, "chan D=512: phase 1 ends on depth"),
    ("lds729", 729, 182, True, "frame N<=1020: one-wave LDS loop of introselect2"),
    ("coop1024", 1024, 512, True, "frame N>1020: cooperative loop of introselect2"),
    ("chan3584", 3584, 1792, True, "chan D=3584"),
    ("chan4096", 4096, 2048, True, "chan D=4096"),
    ("coop8192", 8192, 4096, True, "frame N>1020 / chan D=8192: cooperative loop, 13 index bits"),
]
# per-frame shapes get a second, different killer with its own budget (frame 3 of the five-frame test)
SECOND = ("tail64", "solo196", "solo324", "lds729", "coop1024", "coop8192")
# (name, n, k): std::sort(q, q + k - 1) after nth_element
SORT = [
    ("sort100", 128, 101),
    ("sort400", 512, 401),
    ("sort1792", 3584, 1792),
    ("sort4096", 8192, 4096),
    ("sort6000", 8192, 6000),
]
# fused-pass inputs: (name, F, N, D, dtype, which adversary); k = D / 2 (channel ratio 0.5)
PASS = [
    ("pass512s", 4, 16, 512, "bf16", "select"),
    ("pass512o", 4, 16, 512, "bf16", "sort"),
    ("pass3584s", 2, 49, 3584, "bf16", "select"),
    ("pass3584o", 2, 49, 3584, "bf16", "sort"),
    ("pass4096s", 3, 36, 4096, "f16", "select"),
    ("pass4096o", 3, 36, 4096, "f16", "sort"),
]


def topk_all_dtypes(ranks, k, srt):
    """torch.topk per dtype (the reference), == the oracle; the rules are monotonic, so all dtypes must agree."""
    import oracle as O
    outs = []
    for dn in DTYPES:
        t = rank_values(ranks, dn)
        idx = torch.topk(t, k, largest=False, sorted=srt).indices
        assert torch.equal(O.topk_smallest(t, k, srt), idx), ("oracle topk mismatch", dn, k, srt)
        outs.append(idx.numpy())
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
    return outs[0]


def pass_case(name, F, N, D, dn, how):
    """Amplitude ranks whose channel variances make torch.topk(var, D / 2) meet the selection's depth limit (how = "select")
    or the sort's (how = "sort"): the variances must carry the rank pattern -- same order, same ties -- in the input dtype AND
    in fp32 (the fp32-scored pass), and the transcription run on them must report the limit."""
    import oracle as O
    k = D // 2

    def candidates():
        if how == "select":
            yield search_select(D, k, True)[0], None
        else:
            for seed in range(1, 40):
                rank, _, _ = antiqs_sort(D, k, seed)
                _, c0 = certified(rank.astype(np.uint16), k, True)
                for off in (0, 1):
                    yield tie(rank, k, off), c0["segs"]

    for r, segs0 in candidates():
        x = pass_input(r, F, N, dn)
        var = x.var(0, unbiased=False)
        var32 = x.float().var(0, unbiased=False)
        dense = np.unique(r, return_inverse=True)[1]
        if not all(np.array_equal(np.unique(v.float().numpy(), return_inverse=True)[1], dense) for v in (var, var32)):
            continue
        ok, info = sort_conditions(dense.astype(np.uint16), k)
        if how == "select" and not (info["hit"] and 0 < info["kept"] < info["group"]):
            continue
        if how == "sort" and not (ok and info["segs"] == segs0 and max(l - f for f, l in segs0) > 64):
            continue
        for v in (var, var32):                    # the certified comparisons, on the variances themselves
            vf = v.float().numpy()
            p_real, _ = real(vf, k, True)
            p_tr, cert = trace(vf, k, True)
            assert np.array_equal(p_real, p_tr) and cert["segs"] == info["segs"] and cert["hit"] == info["hit"]
            want = torch.topk(v, k, largest=False).indices
            assert np.array_equal(want.numpy(), p_real[:k])
        idx, ovar = O.select_low_var_channel_idx(x, 0.5)
        assert torch.equal(idx, want) and torch.equal(ovar, var), "oracle channel order / variance"
        return r, info, want.numpy()
    raise SystemExit(f"{name}: no certified pass input")


def write_npz(path, arrays):
    """np.savez_compressed with fixed member times: the file is reproducible byte for byte."""
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def main():
    names, kinds, ns, ks, sorteds, ranks, outs, offs_v, offs_o = [], [], [], [], [], [], [], [0], [0]
    hits, lens, groups, kepts, naives, segs, seg_off, seg_dup, disorders = [], [], [], [], [], [], [0], [], []
    pops_, flips_ = [], []

    def add(name, kind, r, k, srt, out, hit, ln, g, m, naive, sg=(), dup=(), disorder=False, pops=0, flip=False):
        pops_.append(pops); flips_.append(int(flip))
        names.append(name); kinds.append(kind); ns.append(r.size); ks.append(k); sorteds.append(int(srt))
        ranks.append(r.astype(np.uint16)); outs.append(out.astype(np.uint16))
        offs_v.append(offs_v[-1] + r.size); offs_o.append(offs_o[-1] + out.size)
        hits.append(int(hit)); lens.append(ln); groups.append(g); kepts.append(m); naives.append(int(naive))
        for (f, l) in sg:
            segs.append((f, l))
        seg_dup.extend(int(d) for d in dup)
        seg_off.append(seg_off[-1] + len(sg)); disorders.append(int(disorder))

    for (name, n, k0, want_hit, what) in SELECT:
        for which in ([0, 1] if name in SECOND else [0]):
            k = second_k(n, k0) if which else k0
            r, _, var = search_select(n, k, want_hit, seed=1 + which)
            perm, cert, g, m, naive = check_select(name, r, k, want_hit)
            out = topk_all_dtypes(r, k, False)
            assert sorted(out.tolist()) == sorted(perm[:k].tolist())
            nm = name + ("b" if which else "")
            add(nm, 0, r, k, False, out, cert["hit"], cert["len"], g, m, naive, pops=cert["pops"], flip=cert["flip"])
            print(f"select {nm:10s} n={n:5d} k={k:5d} dtypes=bf16,f16,f32  fall-back range={cert['len'] if cert['hit'] else 'none':>5} "
                  f"partitions={cert['parts']:2d} heap-select took in {cert['pops']:4d}  boundary group={g} (kept {m})  beats both naive "
                  f"tie rules={naive}  a wrong heap step changes the set={cert['flip']}  variant(off,a,b)={var}  [{what}]")
    for (name, n, k) in SORT:
        r, info, var = search_sort(n, k, range(1, 40))
        out = topk_all_dtypes(r, k, True)
        add(name, 1, r, k, True, out, info["hit"], info["len"], info["group"], info["kept"], info["naive"], info["segs"],
            info["dup"], info["disorder"])
        print(f"sort   {name:10s} n={n:5d} k={k:5d} dtypes=bf16,f16,f32  heap-sorted segments={[l - f for f, l in info['segs']]} "
              f"dup={info['dup']} tied out of index order={info['disorder']}  select fall-back range="
              f"{info['len'] if info['hit'] else 'none'}  boundary group={info['group']}  (seed, off, free)={var}  [chan ORDER]")
    for (name, F, N, D, dn, how) in PASS:
        r, info, out = pass_case(name, F, N, D, dn, how)
        add(name, 2, r, D // 2, True, out, info["hit"], info["len"], info["group"], info["kept"], info["naive"], info["segs"],
            info["dup"], info["disorder"], pops=info["pops"])
        print(f"pass   {name:10s} F={F} N={N} D={D} {dn}  heap-sorted segments={[l - f for f, l in info['segs']]} "
              f"select fall-back range={info['len'] if info['hit'] else 'none'}  boundary group={info['group']} (kept {info['kept']})  "
              f"beats both naive tie rules={info['naive']}  [k_var_select / ORDER riders in the fused pass]")
    sel_naive = [nm for nm, kd, nv in zip(names, kinds, naives) if kd == 0 and nv]
    print("select fixtures that differ from both naive tie rules:", sel_naive)
    # every engine class: its first killer beats both naive tie rules and notices a wrong heap step
    for nm, kd, nv, fl, ht in zip(names, kinds, naives, flips_, hits):
        if kd == 0 and not nm.endswith("b") and not (nv and (fl or not ht)):
            raise SystemExit(f"{nm}: the reference's choice is a naive tie rule's, or a wrong heap step goes unnoticed")
    arrays = dict(
        names=np.array(names), kind=np.array(kinds, np.int8), n=np.array(ns, np.int32), k=np.array(ks, np.int32),
        sorted=np.array(sorteds, np.int8), ranks=np.concatenate(ranks), out=np.concatenate(outs),
        offs_v=np.array(offs_v, np.int64), offs_o=np.array(offs_o, np.int64),
        sel_hit=np.array(hits, np.int8), sel_len=np.array(lens, np.int32), group=np.array(groups, np.int32),
        group_kept=np.array(kepts, np.int32), naive_differs=np.array(naives, np.int8),
        seg=np.array(segs, np.int32).reshape(-1, 2), seg_off=np.array(seg_off, np.int32), seg_dup=np.array(seg_dup, np.int8),
        disorder=np.array(disorders, np.int8), sel_pops=np.array(pops_, np.int32), flip_differs=np.array(flips_, np.int8),
        pass_shape=np.array([(F, N, D, DTYPES.index(dn)) for (_, F, N, D, dn, _h) in PASS], np.int32),
        start=np.array([START[d] for d in DTYPES], np.int64))
    path = os.path.join(HERE, "depth_limit_kat.npz")
    write_npz(path, arrays)
    print("wrote", path, os.path.getsize(path), "bytes;", len(names), "rank patterns")


if __name__ == "__main__":
    main()

"""Workspaces and output tensors with guard bands, and a patch that hands them to every allocation site of the package
(not a conftest) -- TEST ONLY.

Every entry point of the library takes a caller-owned workspace of vc2_workspace_bytes and promises that (1) the bytes it
finds there do not matter (sweep-1 partials under VC2_FLAG_HAVE_STATS excepted) and (2) it writes only inside the
workspace and inside the outputs' stated extents.  A fresh `torch.empty` is very often zero pages or the same plan's
leftovers, and an overrun into a neighbouring torch allocation shows nowhere, so neither promise is visible to a test that
allocates the ordinary way.  Here a buffer is

    [ guard G bytes | the exactly sized region, filled per `pattern` | guard G bytes ]

with G = max(1 MiB, nbytes) rounded up to 4096: an overrun shorter than a whole workspace stays inside this allocation,
where `intact()` finds it.  The region's base is 4096-aligned, so every alignment rule of the ABI holds.

Patterns, each something `torch.empty` can legitimately return:
    zero      the comparison baseline
    ff        bytes 0xFF: counters read -1, floats and doubles read NaN, the variance array reads "not written yet"
    one       bytes 0x01: counters read 0x01010101 (a "full" queue for every `<` test), floats read tiny normals
    leftover  the workspace bytes a complete pass of ANOTHER clip, shape, dtype and mode left behind (debug mode 2 on a
              `cancel` input: every queue and list full), so that regions land on other regions' offsets
"""
from __future__ import annotations

import contextlib
import ctypes

import torch

from vidcom2_amd import _ffi, synth
from vidcom2_amd.vidcom2 import OutputSet

GUARD_BYTE = 0xA5
PATTERNS = ("zero", "leftover", "ff", "one")          # (leftover runs before ff and one)
_FILL = {"zero": 0x00, "ff": 0xFF, "one": 0x01, "leftover": 0x5A}     # leftover: the OUTPUTS' fill (a workspace takes the donor's bytes)
DONOR = (32, 130, 2048, torch.float16, 9300, "cancel")               # F, N, D, dtype, seed, dist of the leftover donor
_donor_bytes = {}

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
# every (F, N, D, dtype) tests/test_workspace_contract_gpu.py asks a workspace for (the fused cases, the stage wrappers' (1, R, D)
# and (F, N, C), the chunked stages): tests/test_workspace_bytes.py checks on the host that the donor's workspace is at least
# as large as each and that each size is the same in every numerics mode
SHAPES = [(4, 49, 256, BF16), (4, 49, 256, F16), (6, 196, 1024, BF16), (6, 196, 1024, F16), (3, 17, 1024, BF16),
          (3, 17, 1024, F16), (4, 64, 1024, F16), (4, 64, 3584, BF16), (5, 50, 100, F16), (1, 8, 512, BF16),
          (16, 1, 64, BF16), (16, 1, 64, F16), (3, 50, 96, F32), (2, 33, 4104, BF16), (1024, 4, 64, BF16),
          (1025, 4, 64, BF16), (2, 49, 256, BF16), (1, 196, 256, BF16), (4, 49, 128, BF16), (1, 196, 256, F16),
          (4, 49, 128, F16), (7, 49, 256, BF16), (5, 5, 128, F16), (1, 5, 128, F16)]


def _round_up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


class Guarded:
    """One guarded buffer: `view` is the middle (uint8 [nbytes]); `intact()` compares both guards with torch.equal."""

    def __init__(self, nbytes: int, device):
        self.nbytes = int(nbytes)
        self.G = _round_up(max(1 << 20, self.nbytes), 4096)
        self.buf = torch.empty(self.G + self.nbytes + self.G + 4096, dtype=torch.uint8, device=device)
        self.off = (-self.buf.data_ptr()) % 4096 + self.G              # (the middle's base: 4096-aligned)
        self.buf.fill_(GUARD_BYTE)
        self.view = self.buf[self.off: self.off + self.nbytes]
        self._want = torch.full((self.G,), GUARD_BYTE, dtype=torch.uint8, device=device)
        assert self.view.data_ptr() % 4096 == 0

    def guards(self):
        return self.buf[self.off - self.G: self.off], self.buf[self.off + self.nbytes: self.off + self.nbytes + self.G]

    def intact(self) -> bool:
        lo, hi = self.guards()
        return bool(torch.equal(lo, self._want)) and bool(torch.equal(hi, self._want))

    def damage(self) -> str:
        """Where the guards differ, for a failure message: byte offsets relative to the region's ends."""
        lo, hi = self.guards()
        out = []
        for name, g, rel in (("below", lo, -self.G), ("above", hi, self.nbytes)):
            bad = (g != GUARD_BYTE).nonzero().flatten()
            if bad.numel():
                out.append(f"{bad.numel()} bytes {name} the region, offsets {int(bad[0]) + rel}..{int(bad[-1]) + rel}")
        return "; ".join(out) or "intact"


def leftover_bytes(device) -> torch.Tensor:
    """The donor pass's workspace after it ran to the end (made once per process and device, never changed)."""
    key = str(device)
    if key not in _donor_bytes:
        from vidcom2_amd.vidcom2 import CompressPlan
        F, N, D, dt, seed, dist = DONOR
        lib = _ffi.lib()
        before = lib.vc2_get_mode()
        assert lib.vc2_set_mode(2) == 0                                # debug: every value is replayed, every list is full
        try:
            ws = torch.empty(_ffi.workspace_bytes(F, N, D, dt), dtype=torch.uint8, device=device)
            plan = CompressPlan(F, N, D, dt, device, 0.25, want_scores=True, ws=ws)
            plan.enqueue(synth.make(F, N, D, dt, seed, dist).to(device))
            plan.finish()
            torch.cuda.synchronize()
        finally:
            assert lib.vc2_set_mode(before) == 0
        _donor_bytes[key] = ws.clone()
    return _donor_bytes[key]


def fill(view: torch.Tensor, pattern: str) -> None:
    """Fill a uint8 view per `pattern` (the donor's bytes from offset 0, so that its regions meet other offsets; repeated
    if the view is longer than the donor's workspace)."""
    if pattern != "leftover":
        view.fill_(_FILL[pattern])
        return
    donor = leftover_bytes(view.device)
    n = view.numel()
    for o in range(0, n, donor.numel()):
        m = min(donor.numel(), n - o)
        view[o: o + m].copy_(donor[:m])


def guarded(nbytes: int, pattern: str, device):
    """(the middle view, uint8 [nbytes], filled per `pattern`; the Guarded object with `intact()`)."""
    g = Guarded(nbytes, device)
    fill(g.view, pattern)
    return g.view, g


def guarded_tensor(shape, dtype, device, pattern: str):
    """A tensor of exactly `shape` inside guards, its interior pre-filled with the pattern's byte: (tensor, Guarded)."""
    numel = 1
    for s in shape:
        numel *= int(s)
    g = Guarded(numel * torch.empty(0, dtype=dtype).element_size(), device)
    g.view.fill_(_FILL[pattern])
    return g.view.view(dtype).view(*shape), g


def guarded_outputs(plan, pattern: str):
    """An OutputSet for `plan.enqueue(out=...)`: each of idx, ks, rows, v, f, kout a view of its exact extent into a
    guarded buffer, pre-filled.  Returns (OutputSet, [Guarded, ...])."""
    dev, gs = plan.device, []

    def mk(shape, dt, on=True):
        if not on:
            return None
        t, g = guarded_tensor(shape, dt, dev, pattern)
        gs.append(g)
        return t
    out = OutputSet(mk((plan.cap,), torch.int64), mk((plan.F,), torch.int64),
                    mk((plan.cap + plan.tail_rows, plan.D), plan.dtype, plan._gather),
                    mk((plan.F, plan.N), plan.arith_dtype, plan._want_scores),
                    mk((plan.F, plan.N), plan.arith_dtype, plan._want_scores), mk((2,), torch.int64))
    return out, gs


class Recorder:
    """What `patched_workspace` handed out."""

    def __init__(self):
        self.guards = []

    def intact(self) -> bool:
        return all(g.intact() for g in self.guards)

    def damage(self) -> str:
        return " | ".join(f"workspace {i} ({g.nbytes} bytes): {g.damage()}" for i, g in enumerate(self.guards)
                          if not g.intact()) or "intact"


def clear_caches() -> None:
    from vidcom2_amd import chunked, vidcom2
    vidcom2.clear_plan_cache()
    chunked.clear_chunk_cache()


@contextlib.contextmanager
def patched_workspace(monkeypatch, pattern: str):
    """Inside: `vidcom2_amd._ffi.workspace` hands out guarded, patterned views of exactly vc2_workspace_bytes and records
    them.  Every allocation site calls it through the module (CompressPlan, HipStages, fused.pool_stats,
    _channel_variance, compute_gaussian_scores), so the one patch reaches them all; a view takes attributes like any tensor
    (pool_stats' `_vc2_stats_for` tag).  The plan cache and the chunk cache are cleared on the way in and out."""
    rec = Recorder()

    def workspace(F, N, D, dtype, device):
        view, g = guarded(_ffi.workspace_bytes(F, N, D, dtype), pattern, device)
        rec.guards.append(g)
        return view
    clear_caches()
    with monkeypatch.context() as mp:
        mp.setattr(_ffi, "workspace", workspace)
        try:
            yield rec
        finally:
            torch.cuda.synchronize()
            clear_caches()


def selftest_counters():
    out = (ctypes.c_int32 * 8)()
    _ffi.check(_ffi.lib().vc2_selftest_counters(out, 0), "vc2_selftest_counters")
    return list(out)

"""Frame-sharded VidCom2 compression across the GPUs of one node.

One process per GPU (torch.distributed, backend "nccl" = RCCL over xGMI).  Rank p holds a contiguous run of frames
of ONE video: [p*F_local, (p+1)*F_local) with equal shards, [f0_p, f0_p + F_p) with unequal ones (any F_p >= 1;
shard_frames() proposes a split).  The pass shards by frame with three tiny exchange steps --
every message is <= a few hundred KB, i.e. latency-bound, so each is a single all-gather followed by
a fixed-order local reduction (NOT an all-reduce: the fixed order makes every rank compute the same
bits; the partials are CANONICAL -- cut at fixed frame boundaries and folded in one fixed order -- so the bits are also
the same for every world size and every split, and the same as the unsharded pass's, when each rank holds a multiple
of 16 frames; with other splits the fp64 partials are cut elsewhere: every rank still has the same bits, the variances
and centre sums equal the unsharded pass's up to fp64 rounding BEFORE they are rounded to T):

  after sweep 1   per 8-frame block statistics (mean, M2)  fp64 [F_l/8, 2, D] -> identical channel mask
  after sweep 2   per 16-frame sums of normalised tokens   fp64 [F_l/16, C]   -> identical video centre
  after sweep 3   per-frame uniqueness scores  -mean(v)    fp32 [F_local] -> global softmax budgets
                  (the RCCL all-gather BASELINE.json's north_star names)

With unequal shards an exchange whose per-rank size differs (stat blocks, group sums, replay records, s) is padded to
the largest rank's message -- the all-gather stays one rectangular collective -- and compacted on the device before the
stage that consumes it; equal shards issue exactly the calls they always did.

Kept rows stay sharded by frame (each rank returns the kept rows / indices of its own frames); the
reference has no multi-GPU form of this path -- its only parallelism is document-level DP in the
harness (lmms-eval/lmms_eval/evaluator.py:488-491), which is the "replicas only" case.

The arithmetic lives behind a small stage interface so that the collective logic can be exercised on
CPU with gloo (tests inject an oracle-backed stage object); the default stages are the HIP kernels.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch
import torch.distributed as dist

from . import _ffi
from ._ffi import DTYPE_CODE, check, lib, on_device, ptr, stream_ptr


def shard_frames(F_total: int, world: int, align: int = 8) -> list:
    """Frames per rank of a contiguous, balanced split of F_total frames over `world` ranks, every rank >= 1 frame.
    When F_total >= align * world all ranks but the last hold a multiple of `align` frames (align = 8 keeps the
    canonical stat blocks at 8 frames: the channel variances are then the unsharded pass's bits); otherwise the plain
    balanced split (the first F_total % world ranks hold one frame more)."""
    F_total, world, align = int(F_total), int(world), int(align)
    if world < 1 or align < 1:
        raise ValueError(f"shard_frames: world and align must be positive (got {world}, {align})")
    if world > F_total:
        raise ValueError(f"shard_frames: {world} ranks for {F_total} frames -- a rank without frames is not supported")
    if F_total >= align * world:
        units, extra = divmod(F_total // align, world)          # whole `align`-frame units, dealt out evenly
        parts = [(units + (1 if p < extra else 0)) * align for p in range(world)]
        parts[-1] += F_total % align
    else:
        q, r = divmod(F_total, world)
        parts = [q + (1 if p < r else 0) for p in range(world)]
    return parts


def stat_block_frames(frames) -> int:
    """Frames per stat block of exchange 1: the largest power of two <= 8 that divides EVERY rank's frame count, so that
    every f0 is a multiple of it and the gathered blocks form one uniform grid of the video."""
    return next(b for b in (8, 4, 2, 1) if all(f % b == 0 for f in frames))


def pad_rows(t: torch.Tensor, n_max: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """t [n, ...] as the first rows of a zero-padded [n_max, ...] message (t itself when n == n_max)."""
    if t.shape[0] == n_max:
        return t
    if out is None:
        out = torch.zeros((n_max,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[: t.shape[0]].copy_(t)
    return out


def compact_index(counts, device) -> torch.Tensor:
    """Row numbers, in rank order, of the ranks' real rows in a gathered [world * max(counts), ...] buffer."""
    n_max = max(counts)
    return torch.tensor([p * n_max + i for p, c in enumerate(counts) for i in range(c)], dtype=torch.int64, device=device)


def compact_rows(gathered: torch.Tensor, index: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[world, n_max, ...] (padded messages in rank order) -> [sum(counts), ...]: one device gather, no host sync."""
    flat = gathered.reshape((-1,) + tuple(gathered.shape[2:]))
    return torch.index_select(flat, 0, index) if out is None else torch.index_select(flat, 0, index, out=out)


class _CShardOpts(ctypes.Structure):
    """include/vc2.h: vc2_shard_opts."""
    _fields_ = [("params", ctypes.c_void_p), ("score_dtype", ctypes.c_int32), ("tail_records", ctypes.c_int32)]


VC_EDGE, VC_EDGE_TAIL = 64, 256      # raw edge values per side of an exchange-2b record: narrow / wide layout (vc2.h)


def tail_columns(C: int) -> int:
    """Video-centre columns torch sums with row_sum's four interleaved chains: the last C % 32 in torch.topk's order
    (C % 4 when C < 8)."""
    return int(C) % (32 if C >= 8 else 4)


@dataclass
class ShardResult:
    rows: Optional[torch.Tensor]     # [K_local, D] kept rows of this rank's frames
    local_idx: torch.Tensor          # int64 [K_local]  f_local*N + n
    global_idx: torch.Tensor         # int64 [K_local]  index into the whole video's [F_total*N] tokens
    ks: torch.Tensor                 # int64 [F_local]
    K: int


class HipStages:
    """The five shard-local stages on the HIP kernels (include/vc2.h 'frame-sharded building blocks')."""

    def __init__(self, F: int, N: int, D: int, dtype, device, base_scale: float, gather: bool = True,
                 vc_cap: int = 64, frames=None, rank: int = 0, params=None, score_dtype=None, shared=None):
        """frames / rank: the layout of the video over the ranks (every rank's frame count, this rank's number).  None,
        or equal counts: the equal-shard pass (F_total = world * F, set by ShardedCompressor).  Unequal counts: the buffers
        that take part in an exchange are sized for the largest rank and exchange 2b goes through the ragged entry points.
        params (a PassParams) / score_dtype: as in `compress`.  None, a set equal to the reference's defaults and
        score_dtype == dtype are the plain pass: the same entry points with the same arguments.  Bad sets raise here, as
        CompressPlan raises them (ValueError / NotImplementedError), before any collective.
        shared: externally owned buffers by attribute name (stats, csum, blocks, total, s, var_f32, mask, cols, perm, spos), each
        of the shape and dtype this object would allocate: the stage then writes its partials there instead of into
        buffers of its own (chunked.py hands over views of whole-video buffers, so that its "exchanges" copy nothing).
        Two more are optional and never allocated here: v, f ([F, N] in the dtype the pass scores in) -- sweep 3 then
        also writes this rank's video / frame scores there (v_T / f_T of the phase-2 entry points).
        None: every buffer is allocated here, as it always was."""
        from .vidcom2 import _c_params, _norm_params, _norm_score_dtype
        ext = dict(shared or {})

        def buf(name, shape, dt, zero=False):
            t = ext.pop(name, None)
            if t is None:
                return (torch.zeros if zero else torch.empty)(shape, dtype=dt, device=self.device)
            if tuple(t.shape) != tuple(shape) or t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"HipStages: shared buffer {name!r} must be a contiguous {dt} {tuple(shape)} tensor on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            return t
        self.params = _norm_params(params)
        # fp32 scoring of bf16 / fp16 rows: 16-bit loads, fp32 variances, scores and selection; no "torch order" replay
        self.score32 = _norm_score_dtype(score_dtype, dtype) is not None
        self._cparams = _c_params(self.params, D)              # (raises for a channel count of 0 or above the sweeps' limit)
        self.F, self.N, self.D, self.dtype, self.device, self.base = F, N, D, dtype, torch.device(device), base_scale
        self.code = DTYPE_CODE[dtype]
        L = lib()
        self.frames = [int(f) for f in frames] if frames is not None else None
        self.rank = int(rank)
        self.ragged = self.frames is not None and len(set(self.frames)) > 1
        if self.frames is not None and (not 0 <= self.rank < len(self.frames) or self.frames[self.rank] != F
                                        or min(self.frames) < 1):
            raise ValueError(f"HipStages: rank {rank} with {F} frames does not fit the layout {self.frames}")
        self.ws = _ffi.workspace(F, N, D, dtype, self.device)
        # canonical partials: per stat block of `bf` frames (mean, M2); per group of 16 frames the
        # sums of the normalised tokens.  bf = 8 whenever F is a multiple of 8 (then the gathered blocks are exactly
        # the unsharded pass's blocks and every world size reduces to the same bits); unequal shards: the largest
        # power of two that divides every rank's count
        self.bf = stat_block_frames(self.frames if self.ragged else [F])
        self.stats = buf("stats", (F // self.bf, 2, D), torch.float64)
        self.C = int(self._cparams.channels) if self._cparams is not None else int(D * 0.5)   # int(x.shape[-1] * ratio), vidcom2.py:41
        # exchange 2: per group of 16 frames the sums of x^ and, behind them, the groups' bounds of sum |x^|.  Unequal
        # shards: k_video_centre reads every rank's message as [half sums | half bounds], so a rank with fewer groups
        # than the largest pads INSIDE each half (zero rows: they change neither the sums nor the bounds)
        G = (F + 15) // 16
        self._G, self._Gmax = G, max((f + 15) // 16 for f in self.frames) if self.ragged else G
        self.csum = buf("csum", (2 * self._Gmax, self.C), torch.float64, zero=True)     # (a shared one: zeroed by its owner)
        self._csum_raw = (torch.empty((2 * G, self.C), dtype=torch.float64, device=self.device)
                          if G != self._Gmax else self.csum)
        self.F_total = sum(self.frames) if self.ragged else F   # equal shards: set by ShardedCompressor (world * F)
        # the layout as the ragged entry points take it: a host array of the ranks' row counts
        self._rank_rows = (ctypes.c_int64 * len(self.frames))(*[f * N for f in self.frames]) if self.ragged else None
        self.var_f32 = buf("var_f32", (D,), torch.float32)
        self.mask = buf("mask", (D,), torch.uint8)
        self.cols = buf("cols", (D,), torch.int32)
        self.perm = buf("perm", (D,), torch.int32)                            # channels as nth_element left them
        self.spos = buf("spos", (D,), torch.int32)                            # their positions in that order
        # phase 1 replays torch.topk's channel ORDER (perm -> spos) in a rider workgroup of sweep 2.  Stages that share one
        # spos (chunked.py) need it once: the others are told that spos is valid already (perm == NULL, include/vc2.h)
        self.order_rider = True
        self.total = buf("total", (F * N,), torch.float32)
        self.s = buf("s", (F,), torch.float32)
        sdt = torch.float32 if self.score32 else dtype
        self.v = buf("v", (F, N), sdt) if "v" in ext else None
        self.f = buf("f", (F, N), sdt) if "f" in ext else None
        # a rank can hold the globally dominant frame: sum of its scales <= base * (F_local + 1)
        self.cap = min(F * N, int(L.vc2_kept_capacity(F + 1, N, base_scale)))
        self.idx = torch.empty(self.cap, dtype=torch.int64, device=self.device)
        self.ks = torch.empty(F, dtype=torch.int64, device=self.device)
        self.kout = torch.zeros(4, dtype=torch.int64, device=self.device)     # K, capacity overflow, fragile centre columns
        # exchange 2b (video-centre replay): level-0 block sums of this rank's rows for up to vc_cap flagged columns
        self.vc_cap = int(vc_cap)                             # flagged columns whose blocks one exchange carries
        self.vc_replay = dtype != torch.float32 and not self.score32
        # per flagged column: 64 + 64 raw edge values and the sums of this rank's complete blocks (include/vc2.h)
        # (unequal shards: every rank's records have the stride of the rank with the most rows)
        # The C % 32 tail columns (row_sum's four interleaved chains) need the WIDE layout: 256 + 256 raw edge values and
        # four sums per complete run; then every column of the pass, plain ones included, is exchanged in it
        self.vc_tail = self.vc_replay and tail_columns(self.C) > 0
        self.vc_edge = VC_EDGE_TAIL if self.vc_tail else VC_EDGE
        self.blocks = buf("blocks", (self.vc_cap, 2 * self.vc_edge + 1 + (max(self.frames) if self.ragged else F) * N // 16),
                          torch.float32, zero=True)
        # the options of the `_o` entry points; None: the plain symbols, today's calls
        self._opts = None
        if self._cparams is not None or self.vc_tail or self.score32:
            self._opts = _CShardOpts(ctypes.addressof(self._cparams) if self._cparams is not None else None,
                                     DTYPE_CODE[torch.float32] if self.score32 else self.code, 1 if self.vc_tail else 0)
        self.rows = torch.empty((self.cap, D), dtype=dtype, device=self.device) if gather else None
        if ext:
            raise ValueError(f"HipStages: unknown shared buffer(s) {sorted(ext)}")

        # device pointers of the fixed buffers, resolved once: the per-pass host work is five C calls plus
        # three collectives, and that host time bounds the pass when it exceeds the ~0.3 ms of GPU work
        self._L = L
        self._p = {n: ptr(getattr(self, n)) for n in ("ws", "stats", "csum", "var_f32", "mask", "cols", "perm",
                                                     "spos", "total", "s", "idx", "ks", "kout", "rows", "blocks",
                                                     "_csum_raw", "v", "f")}
        self._ws_n = self.ws.numel()

    def _call(self, name: str, *args):
        """The entry point `name`, or -- a pass with options -- its `_o` form with them as the trailing argument."""
        if self._opts is None:
            check(getattr(self._L, name)(*args), name)
        else:
            check(getattr(self._L, name + "_o")(*args, ctypes.byref(self._opts)), name + "_o")

    def _st(self):
        return stream_ptr(self.device)

    def set_layout(self, frames, rank) -> None:
        """What ShardedCompressor tells a stage object about unequal shards.  These stages are built for one layout."""
        if [int(f) for f in frames] != self.frames or int(rank) != self.rank:
            raise ValueError(f"HipStages was built for the layout {self.frames} (rank {self.rank}), not {list(frames)} "
                             f"(rank {rank}): pass frames= and rank= to its constructor")

    def set_score_views(self, v, f) -> None:
        """Other tensors for this rank's scores from the next phase 2 on (chunked.py: fresh ones per video), each a
        contiguous [F, N] tensor in the dtype the pass scores in; None, None: no score outputs."""
        sdt = torch.float32 if self.score32 else self.dtype
        for name, t in (("v", v), ("f", f)):
            if t is not None and (tuple(t.shape) != (self.F, self.N) or t.dtype != sdt or t.device != self.device
                                  or not t.is_contiguous()):
                raise ValueError(f"HipStages: score view {name!r} must be a contiguous {sdt} {(self.F, self.N)} tensor on "
                                 f"{self.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
            setattr(self, name, t)
            self._p[name] = ptr(t)

    def chan_stats(self, x):
        p = self._p
        self._call("vc2_chan_stats", ptr(x), self.F, self.N, self.D, self.code, self.F_total, self.bf, p["ws"],
                   self._ws_n, p["stats"], self._st())
        return self.stats

    def select_channels(self, stats_all, R_total):
        p, st = self._p, self._st()
        blocks = stats_all.reshape(-1, 2, self.D)               # [world * nb, 2, D], rank order = frame order
        # (the variance is rounded to the SCORING dtype: fp32 ones go through vc2_chan_select's 64-bit selection words)
        check(self._L.vc2_chan_var_from_stats(ptr(blocks), blocks.shape[0], self.bf * self.N, R_total, self.D,
                                              DTYPE_CODE[torch.float32] if self.score32 else self.code,
                                              None, p["var_f32"], st), "vc2_chan_var_from_stats")
        # the channel SET now; torch.topk's channel ORDER (needed only by the fix-up kernels of phase 1) is
        # replayed from `perm` by a rider workgroup of sweep 2 inside vc2_scores_phase1
        check(self._L.vc2_chan_select(p["var_f32"], self.D, self.C, p["mask"], p["cols"], p["perm"], None, None, None,
                                      st), "vc2_chan_select")

    def phase1(self, x):
        p = self._p
        self._call("vc2_scores_phase1", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C, p["spos"],
                   p["perm"] if self.order_rider else None, p["var_f32"], self.F_total, p["ws"], self._ws_n,
                   p["_csum_raw"], self._st())
        if self._G != self._Gmax:                               # fewer groups than the largest rank: pad inside each half
            self.csum[: self._G].copy_(self._csum_raw[: self._G])
            self.csum[self._Gmax: self._Gmax + self._G].copy_(self._csum_raw[self._G:])
        return self.csum

    def vc_blocks(self, x, csum_all, R_total, f0=0):
        """Exchange 2b: this rank's level-0 block sums (and the raw values of the blocks it shares with its neighbours)
        of the boundary-near video-centre columns, or None when the replay does not apply (fp32, exact mode, more tokens
        than the replay models) -- a decision every rank takes identically.  f0 = the video index of this rank's first
        frame.  A block may meet any number of ranks (since round 4: ranks with fewer rows than a block included)."""
        from .vidcom2 import cascade_modelled
        Rl = self.F * self.N
        if not self.vc_replay or _ffi.get_mode() != "torch" or not cascade_modelled(R_total):
            return None
        p = self._p
        parts = csum_all.reshape(-1, csum_all.shape[-1])
        if self.ragged:
            self._call("vc2_video_centre_blocks_ragged", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C,
                       p["spos"], ptr(parts), parts.shape[0], parts.shape[1], self.csum.shape[0], R_total,
                       self._rank_rows, len(self.frames), self.rank, p["ws"], self._ws_n, p["blocks"], self.vc_cap,
                       self._st())
            return self.blocks
        if R_total % Rl != 0:
            return None
        self._call("vc2_video_centre_blocks", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C, p["spos"],
                   ptr(parts), parts.shape[0], parts.shape[1], self.csum.shape[0], R_total, int(f0) * self.N, p["ws"],
                   self._ws_n, p["blocks"], self.vc_cap, self._st())
        return self.blocks

    def flagged_columns(self) -> int:
        """How many video-centre columns the flag kernel of vc_blocks marked (SYNCHRONISES: one device-to-host read; every
        rank reads the same number -- the flags come from the all-gathered sums).  Only the modes that can flag more
        columns than one exchange carries ask (proven margins, debug)."""
        out = ctypes.c_int32(0)
        check(self._L.vc2_video_centre_flagged(self.F, self.N, self.D, self.code, self.F_total * self.N, self._p["ws"],
                                               self._ws_n, ctypes.byref(out), self._st()), "vc2_video_centre_flagged")
        return int(out.value)

    def needs_rounds(self) -> bool:
        """Modes whose video-centre margins can flag more than vc_cap columns: 3 (proven) and 2 (debug: all of them)."""
        return self.vc_replay and int(self._L.vc2_get_mode()) in (2, 3)

    def vc_blocks_round(self, x, R_total, f0, col_offset):
        p = self._p
        if self.ragged:
            self._call("vc2_video_centre_blocks_round_ragged", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C,
                       p["spos"], R_total, self._rank_rows, len(self.frames), self.rank, p["ws"], self._ws_n, p["blocks"],
                       self.vc_cap, int(col_offset), self._st())
            return self.blocks
        self._call("vc2_video_centre_blocks_round", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C, p["spos"],
                   R_total, int(f0) * self.N, p["ws"], self._ws_n, p["blocks"], self.vc_cap, int(col_offset), self._st())
        return self.blocks

    def vc_finish_round(self, R_total, blocks_all, col_offset):
        p = self._p
        if self.ragged:
            self._call("vc2_video_centre_finish_round_ragged", self.F, self.N, self.D, self.code, self.C, p["spos"], R_total,
                       self._rank_rows, len(self.frames), self.rank, p["ws"], self._ws_n, ptr(blocks_all), self.vc_cap,
                       int(col_offset), self._st())
            return
        self._call("vc2_video_centre_finish_round", self.F, self.N, self.D, self.code, self.C, p["spos"], R_total, p["ws"],
                   self._ws_n, ptr(blocks_all), int(blocks_all.shape[0]), self.vc_cap, int(col_offset), self._st())

    def phase2(self, x, csum_all, R_total, blocks_all=None, vc_final=False):
        """vc_final: the video centre in the workspace is final (vc_blocks + vc_finish_round rounds): sweep 3 only."""
        p = self._p
        parts = csum_all.reshape(-1, csum_all.shape[-1])       # [world * groups, C], rank order = frame order
        world = -1 if vc_final else (0 if blocks_all is None else int(blocks_all.shape[0]))
        if vc_final:
            blocks_all = None
        if self.ragged and blocks_all is not None:
            self._call("vc2_scores_phase2_blocks_ragged", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C,
                       p["spos"], ptr(parts), parts.shape[0], parts.shape[1], self.csum.shape[0], R_total, self._rank_rows,
                       len(self.frames), self.rank, p["ws"], self._ws_n, p["v"], p["f"], p["total"], p["s"], ptr(blocks_all),
                       self.vc_cap, self._st())
            return self.s
        self._call("vc2_scores_phase2_blocks", ptr(x), self.F, self.N, self.D, self.code, p["cols"], self.C, p["spos"],
                   ptr(parts), parts.shape[0], parts.shape[1], self.csum.shape[0], R_total, p["ws"], self._ws_n, p["v"],
                   p["f"], p["total"], p["s"], ptr(blocks_all) if blocks_all is not None else None, world, self.vc_cap,
                   self._st())
        return self.s

    def select(self, x, s_all, f0):
        p = self._p
        self._call("vc2_select_sharded", p["total"], ptr(s_all), s_all.numel(), f0, self.F, self.N, self.D,
                   float(self.base), self.code, p["ws"], self._ws_n, p["ks"], p["idx"], self.cap, p["kout"],
                   ptr(x if self.rows is not None else None), p["rows"], self._st())

    def result(self, f0):
        K, overflow, vc_fragile, _ = self.kout.tolist()     # the path's single host sync
        if overflow:
            from .vidcom2 import _raise_status
            _raise_status(int(overflow), self.cap, int(K))
        self.vc_fragile = int(vc_fragile)
        if vc_fragile and _ffi.get_mode() == "torch":
            import warnings
            warnings.warn(f"vidcom2_amd (frame-sharded pass): {vc_fragile} video-centre value(s) lie within the replay margin "
                          "of a rounding boundary and could not be replayed across ranks "
                          f"(more than {self.vc_cap} such columns in a mode that does not go in rounds); they keep "
                          "the exactly rounded mean, the reference's fp32 summation order could round the other way.",
                          RuntimeWarning, stacklevel=2)
        li = self.idx[:K]
        return ShardResult(self.rows[:K] if self.rows is not None else None, li, li + f0 * self.N, self.ks, int(K))


def _all_gather(t: torch.Tensor, group, world: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[world, *t.shape] stacked in rank order (one all-gather; RCCL on GPU tensors, gloo on CPU).  `out` is a
    preallocated [world, *t.shape] buffer (the hot path passes one; tests may not)."""
    if world == 1:
        return t.unsqueeze(0)
    if out is None:
        out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out.view(-1), t.contiguous().view(-1), group=group)
    return out


class ShardedCompressor:
    """Frame-sharded pass; every rank calls enqueue(x_local) + finish() collectively.  F_local may differ between the
    ranks (>= 1 each; N, D and the dtype must agree).  `frames` holds all ranks' counts, `f0` this rank's first frame,
    `F_total` their sum.

    Stage objects (`stages=`): with equal shards the protocol of HipStages' five methods as it always was.  With unequal
    shards the object must have set_layout(frames, rank) -- called once, here -- and then: chan_stats returns
    [F_local / bf, 2, D] with bf = stat_block_frames(frames) and select_channels takes the compacted [sum F_p / bf, 2, D];
    phase1's and vc_blocks' messages have the same shape on every rank (the stage pads them for the largest rank);
    phase2 returns [F_local] and select takes the compacted [F_total]."""

    def __init__(self, F_local: int, N: int, D: int, dtype, device, base_scale: float = 0.25, group=None,
                 stages=None, gather: bool = True, always_collective: bool = False, params=None, score_dtype=None):
        """params (a PassParams) / score_dtype: as in `compress`; every rank must pass the same (checked here, with the
        geometry).  Defaults, a set equal to them and score_dtype == dtype are the plain pass.  With `stages=` they are only
        checked across the ranks: the injected object computes what it was built for.
        always_collective: issue the all-gathers even at world size 1 (a process group must be initialised) -- the
        only way to put the RCCL exchanges themselves under test on a single-GPU box."""
        self.group = group
        self.always_collective = bool(always_collective)
        self._xev = None                                  # per-exchange hipEvent pairs (profile_exchanges)
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if self.world > 1 else 0
        self.F, self.N, self.D = int(F_local), int(N), int(D)
        if self.F < 1:
            raise ValueError(f"ShardedCompressor: a rank needs at least one frame (got {F_local})")
        self.frames = [self.F] * self.world
        # what the built-in stages would refuse is refused before any collective (an injected stage object: its own business)
        from .vidcom2 import _c_params, _norm_params, _norm_score_dtype
        self.params = _norm_params(params)
        self.score_dtype = _norm_score_dtype(score_dtype, dtype) if isinstance(dtype, torch.dtype) else score_dtype
        if stages is None:
            _c_params(self.params, self.D)
        if self.world > 1:
            # the ranks may bring different numbers of frames, but one frame geometry and one dtype: say so instead of
            # hanging in a mismatched collective
            fl = [None] * self.world
            dist.all_gather_object(fl, (self.F, self.N, self.D, str(dtype), self.params, str(self.score_dtype)), group=group)
            if any(t[1:4] != fl[0][1:4] for t in fl) or any(t[0] < 1 for t in fl):
                raise ValueError("ShardedCompressor: every rank must hold at least one frame and the same (tokens per "
                                 f"frame, width, dtype); got (frames, tokens per frame, width, dtype) = {[t[:4] for t in fl]}")
            if any(t[4:] != fl[0][4:] for t in fl):
                raise ValueError("ShardedCompressor: every rank must pass the same params and score_dtype; got "
                                 f"{[t[4:] for t in fl]}")
            self.frames = [int(t[0]) for t in fl]
        self.ragged = len(set(self.frames)) > 1
        self.F_total = sum(self.frames)
        self.f0 = sum(self.frames[: self.rank])
        if stages is not None:
            self.stages = stages
        elif self.ragged:
            self.stages = HipStages(self.F, self.N, self.D, dtype, device, base_scale, gather, frames=self.frames,
                                    rank=self.rank, params=self.params, score_dtype=score_dtype)
        else:
            self.stages = HipStages(self.F, self.N, self.D, dtype, device, base_scale, gather, params=self.params,
                                    score_dtype=score_dtype)
        if self.ragged:
            # the stage object has to cut its partials for THIS layout (stat blocks, padded group sums, record stride)
            if not callable(getattr(self.stages, "set_layout", None)):
                raise TypeError(f"ShardedCompressor: the ranks hold unequal frame counts {self.frames}, and the stage object "
                                f"{type(self.stages).__name__} has no set_layout(frames, rank) method to take that layout")
            self.stages.set_layout(self.frames, self.rank)
        elif isinstance(self.stages, HipStages):
            self.stages.F_total = self.F_total
        self._bf = stat_block_frames(self.frames)
        self._cidx, self._pad, self._cat = {}, {}, {}

        self._gbuf = {}

    def _gather(self, key: str, t: torch.Tensor) -> torch.Tensor:
        if self.world == 1 and not self.always_collective:
            return t.unsqueeze(0)
        buf = self._gbuf.get(key)
        if buf is None or buf.shape[1:] != t.shape or buf.dtype != t.dtype or buf.device != t.device:
            buf = self._gbuf[key] = torch.empty((self.world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
        if self._xev is None or not t.is_cuda:
            return self._collect(t, buf)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = self._collect(t, buf)
        b.record()
        self._xev.setdefault(key, []).append((a, b))
        return out

    def _gather_rows(self, key: str, t: torch.Tensor, counts) -> torch.Tensor:
        """An exchange whose message differs in size between the ranks (rank p brings counts[p] leading rows): padded to
        the largest, one rectangular all-gather, compacted to [sum(counts), ...] in rank order on the device."""
        n_max = max(counts)
        if t.shape[0] != n_max:
            buf = self._pad.get(key)
            if buf is None or buf.shape[1:] != t.shape[1:] or buf.dtype != t.dtype or buf.device != t.device:
                buf = self._pad[key] = torch.zeros((n_max,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            t = pad_rows(t, n_max, buf)
        got = self._gather(key, t)
        idx = self._cidx.get(key)
        if idx is None or idx.device != t.device:
            idx = self._cidx[key] = compact_index(counts, t.device)
        out = self._cat.get(key)
        if out is None or out.shape[1:] != t.shape[1:] or out.dtype != t.dtype or out.device != t.device:
            out = self._cat[key] = torch.empty((sum(counts),) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
        return compact_rows(got, idx, out)

    def _collect(self, t: torch.Tensor, buf: torch.Tensor) -> torch.Tensor:
        if self.world == 1:                                # (always_collective: the collective itself, one rank)
            dist.all_gather_into_tensor(buf.view(-1), t.contiguous().view(-1), group=self.group)
            return buf
        return _all_gather(t, self.group, self.world, buf)

    def profile_exchanges(self, on: bool = True) -> None:
        """hipEvents around every exchange of the passes that follow (stats / csum / blocks / s)."""
        self._xev = {} if on else None

    def exchange_times_us(self) -> dict:
        """Mean microseconds per exchange since profile_exchanges(True) (synchronises); the message sizes with them."""
        torch.cuda.synchronize()
        out = {}
        for key, evs in (self._xev or {}).items():
            buf = self._gbuf.get(key)
            out[key] = {"us": round(sum(a.elapsed_time(b) for a, b in evs) / len(evs) * 1e3, 1),
                        "bytes_per_rank": int(buf[0].numel() * buf.element_size()) if buf is not None else None}
        return out

    def enqueue(self, x_local: torch.Tensor) -> None:
        st = self.stages
        if isinstance(st, HipStages):
            if x_local.dim() != 2 or tuple(x_local.shape) != (self.F * self.N, self.D) or x_local.dtype != st.dtype \
                    or x_local.device != st.device:
                raise RuntimeError(f"x_local must be a {st.dtype} [{self.F * self.N}, {self.D}] tensor on {st.device}, "
                                   f"got {x_local.dtype} {tuple(x_local.shape)} on {x_local.device}")
            if not x_local.is_contiguous():
                x_local = x_local.contiguous()
            with on_device(st.device):
                return self._enqueue(x_local)
        return self._enqueue(x_local)

    def _enqueue(self, x_local: torch.Tensor) -> None:
        st = self.stages
        R_total = self.F_total * self.N
        if self.ragged:                                                          # exchange 1: [sum nb_p, 2, D] fp64
            stats_all = self._gather_rows("stats", st.chan_stats(x_local), [f // self._bf for f in self.frames])
        else:
            stats_all = self._gather("stats", st.chan_stats(x_local))           # exchange 1: [W, 2, D] fp64
        st.select_channels(stats_all, R_total)
        csum_all = self._gather("csum", st.phase1(x_local))                     # exchange 2: [W, D] fp64
        blocks = st.vc_blocks(x_local, csum_all, R_total, self.f0) if hasattr(st, "vc_blocks") else None
        if blocks is not None and getattr(st, "needs_rounds", lambda: False)():
            # proven-margin / debug modes: as many rounds of exchange 2b as the flagged columns need (one host sync for
            # their count -- identical on every rank, so every rank issues the same collectives)
            n = st.flagged_columns()
            for j0 in range(0, max(n, 1), st.vc_cap):
                if j0:
                    blocks = st.vc_blocks_round(x_local, R_total, self.f0, j0)
                st.vc_finish_round(R_total, self._gather("blocks", blocks), j0)
            s_loc = st.phase2(x_local, csum_all, R_total, vc_final=True)
        elif blocks is not None:                                                 # exchange 2b: [W, vc_cap, 129 (513: wide layout) + R_local/16] fp32
            s_loc = st.phase2(x_local, csum_all, R_total, self._gather("blocks", blocks))
        else:
            s_loc = st.phase2(x_local, csum_all, R_total)
        s_all = self._gather_rows("s", s_loc, self.frames) if self.ragged else self._gather("s", s_loc)   # exchange 3: [W, F_local]
        st.select(x_local, s_all.reshape(-1), self.f0)

    def finish(self) -> ShardResult:
        return self.stages.result(self.f0)

    def __call__(self, x_local: torch.Tensor) -> ShardResult:
        self.enqueue(x_local)
        return self.finish()

    def gather_kept(self, res: ShardResult, dst: Optional[int] = None):
        """All ranks' kept rows in frame order (SURVEY.md §8e "output": the consumer is usually one rank's LLM
        prefill).  Two all-gathers: the per-rank counts, then the rows padded to the largest count (an all-gather-v).
        Returns (rows [K_total, D], global_idx [K_total], counts) on every rank, or only on rank `dst` (None
        elsewhere).  The kept rows stay sharded unless this is called."""
        if res.rows is None:
            raise RuntimeError("gather_kept needs a compressor built with gather=True")
        if self.world == 1:
            return res.rows, res.global_idx, [res.K]
        dev = res.rows.device
        counts = _all_gather(torch.tensor([res.K], dtype=torch.int64, device=dev), self.group, self.world).view(-1)
        counts = [int(c) for c in counts.tolist()]                  # (host sync: sizes of the result)
        kmax = max(counts)
        D = res.rows.shape[1]
        pad_rows = torch.zeros((kmax, D), dtype=res.rows.dtype, device=dev)
        pad_idx = torch.zeros(kmax, dtype=torch.int64, device=dev)
        pad_rows[: res.K] = res.rows
        pad_idx[: res.K] = res.global_idx
        all_rows = _all_gather(pad_rows, self.group, self.world)
        all_idx = _all_gather(pad_idx, self.group, self.world)
        if dst is not None and self.rank != dst:
            return None
        rows = torch.cat([all_rows[r, :c] for r, c in enumerate(counts)])
        gidx = torch.cat([all_idx[r, :c] for r, c in enumerate(counts)])
        return rows, gidx, counts

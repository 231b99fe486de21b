"""One video held as a list of frame chunks, compressed on one GPU without concatenating them.

A vision tower that bounds its activation memory encodes a few dozen frames at a time and yields a list of [F_c * N, D]
tensors.  `compress(torch.cat(chunks), ...)` costs a second allocation of the whole video and a copy of it in front of the
pass; `compress_chunks(chunks, ...)` / `ChunkedCompressor` run the pass on the chunks where they lie.

The arithmetic is the frame-sharded pass's (sharded.py, include/vc2.h "frame-sharded multi-GPU building blocks"): every
chunk is one logical rank -- one `HipStages`, built with the layout -- and the three exchanges are not collectives but
views: every stage writes its partials (stat blocks, padded group sums, exchange-2b records, per-frame scores, token
scores) straight into its slot of ONE whole-video buffer, which the stages that consume them read in place.  The channels
are selected once for all stages (and torch.topk's order of them replayed once, by the first chunk's sweep 2), the budgets and the per-frame selection run once over the whole video
(`vc2_select_chunks`), and the kept rows are gathered from the chunks' allocations into one [K, D] tensor by one launch
(`k_gather_rows_chunks`).

Numerics (the sharded pass's own contract): chunks that are each a multiple of 16 frames give the bits of
`compress(torch.cat(chunks))`.  Other splits give the same channel variances and centre sums up to fp64 rounding before
they are rounded to T; the video-centre replay then goes through the ragged exchange-2b forms.  Leftover fragile
video-centre columns are reported by the same RuntimeWarning as `HipStages.result`.  At most 64 chunks
(VC2_RAGGED_MAX_WORLD).

Not offered here: `grid_vid` / `newline`, score outputs, `pool_stats` workspaces, chunks on different devices.
"""
from __future__ import annotations

import bisect
import ctypes
import warnings
from collections import OrderedDict
from typing import Callable, List, Optional, Sequence

import torch

from . import _ffi
from . import autograd as _ag
from . import vidcom2 as _vc
from ._ffi import DTYPE_CODE, check, lib, on_device, ptr, require_device, stream_ptr
from .sharded import VC_EDGE, VC_EDGE_TAIL, HipStages, stat_block_frames, tail_columns
from .vidcom2 import CompressionResult

MAX_CHUNKS = 64                      # include/vc2.h: VC2_RAGGED_MAX_WORLD

__all__ = ["compress_chunks", "ChunkedCompressor", "chunk_starts", "chunk_of_row", "clear_chunk_cache", "MAX_CHUNKS"]


def chunk_starts(chunk_rows: Sequence[int]) -> List[int]:
    """The chunk table: [0, r_0, r_0 + r_1, ..., sum r] -- chunk c holds rows [starts[c], starts[c + 1]) of the virtual
    torch.cat(chunks)."""
    starts = [0]
    for r in chunk_rows:
        if int(r) < 1:
            raise ValueError(f"a chunk holds {r} rows: every chunk needs at least one")
        starts.append(starts[-1] + int(r))
    return starts


def chunk_of_row(starts: Sequence[int], row: int) -> int:
    """The chunk that holds `row` of the virtual concatenation (what k_gather_rows_chunks finds per kept row)."""
    if not 0 <= row < starts[-1]:
        raise IndexError(f"row {row} is outside [0, {starts[-1]})")
    return bisect.bisect_right(starts, row) - 1


def _check_layout(frames) -> List[int]:
    frames = [int(f) for f in frames]
    if not frames:
        raise ValueError("a chunked video needs at least one chunk (got an empty list)")
    if len(frames) > MAX_CHUNKS:
        raise NotImplementedError(f"{len(frames)} chunks: at most {MAX_CHUNKS} are supported (concatenate neighbours)")
    if min(frames) < 1:
        raise ValueError(f"every chunk needs at least one frame (got the frame counts {frames})")
    return frames


class _GatherChunks(torch.autograd.Function):
    """rows = torch.cat(chunks)[global_idx], made by the chunk gather: the backward hands every chunk the rows of the output
    gradient that came from it (vc2_rows_grad once per chunk, with the chunk's sub-range of the ascending index list) and
    zero rows for its dropped tokens."""

    @staticmethod
    def forward(ctx, box, *chunks):
        ctx.spec = box.spec
        return box.outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        idx, counts, starts, shapes = ctx.spec
        D = int(g.shape[-1])
        g = g.reshape(-1, D)
        out, k0 = [], 0
        for c, n in enumerate(counts):
            rows_c = starts[c + 1] - starts[c]
            if not ctx.needs_input_grad[1 + c]:
                out.append(None)
            elif n == 0:
                out.append(torch.zeros(shapes[c], dtype=g.dtype, device=g.device))
            else:
                local = idx[k0: k0 + n] - starts[c]
                out.append(_ag.rows_grad([g], [rows_c], local, n, dst_row0=k0)[0].view(shapes[c]))
            k0 += n
        return (None,) + tuple(out)


class ChunkedCompressor:
    """The pass over one video that arrives as len(frames) chunks of frames[c] frames each, in frame order.

        cc = ChunkedCompressor(frames, N, D, dtype, device)
        for chunk in producer: cc.add(chunk)      # enqueues only
        res = cc.finish()                         # the pass's single host sync

    `add` enqueues the chunk's sweep 1 on the current stream at once and keeps a reference to the chunk; nothing else can
    run before the last chunk, because the channel mask needs all of them.  The LAST `add` enqueues the rest of the pass
    (sweeps 2 and 3 per chunk, one selection, one gather).  Neither synchronises with the host, except where
    ShardedCompressor._enqueue does: the proven-margin and debug modes read the number of flagged video-centre columns once.
    `finish` synchronises once and returns CompressionResult(rows [K, D], global_idx, ks [F_total], K); global_idx indexes
    the virtual torch.cat(chunks), rows is None with gather=False.  The object serves one video at a time and is reusable
    for the next video of the same layout; every video gets fresh output tensors.  Numerics: see the module docstring.

    stages_factory(F_c, N, D, dtype, base_scale, frames, rank) -> a stage object with ShardedCompressor's protocol (tests
    inject CPU stages): the driver then exchanges by torch.cat / torch.stack and selects per chunk.  None: the HIP stages
    on shared whole-video buffers, `vc2_select_chunks` and the chunk gather.
    """

    def __init__(self, frames, N: int, D: int, dtype, device, base_scale: float = 0.25, gather: bool = True,
                 params=None, score_dtype=None, stages_factory: Optional[Callable] = None, vc_cap: int = 64):
        self.frames = _check_layout(frames)
        self.N, self.D, self.dtype, self.device = int(N), int(D), dtype, torch.device(device)
        self.base, self.gather = float(base_scale), bool(gather)
        # bad params / score_dtype: exactly what HipStages raises, before a stage exists
        self.params = _vc._norm_params(params)
        self.score32 = _vc._norm_score_dtype(score_dtype, dtype) is not None
        cparams = _vc._c_params(self.params, self.D)
        W = len(self.frames)
        self.F_total = sum(self.frames)
        self.f0s = [sum(self.frames[:c]) for c in range(W)]
        self.starts = chunk_starts([f * self.N for f in self.frames])
        self._hip = stages_factory is None
        self._chunks: List[torch.Tensor] = []
        self._user_chunks: List[torch.Tensor] = []           # as handed over (autograd attaches to these)
        self._stat_parts: List[torch.Tensor] = []
        self._pending = None
        if not self._hip:
            self.stages = [stages_factory(f, self.N, self.D, dtype, self.base, list(self.frames), c)
                           for c, f in enumerate(self.frames)]
            for c, s in enumerate(self.stages):
                if callable(getattr(s, "set_layout", None)):
                    s.set_layout(list(self.frames), c)
            return
        if self.device.type != "cuda":
            raise RuntimeError(f"vidcom2_amd: a chunked video on {self.device}; this package only runs its HIP kernels on a "
                               "ROCm device (torch device type 'cuda'). There is no CPU fallback.")
        dev, N, D = self.device, self.N, self.D
        self._L = lib()
        # the whole-video buffers the stages' "exchanges" are views of (sizes: HipStages checks each view against its own)
        bf = stat_block_frames(self.frames)
        nbs = [f // bf for f in self.frames]
        C = int(cparams.channels) if cparams is not None else int(D * 0.5)
        Gmax = max((f + 15) // 16 for f in self.frames)
        replay = dtype != torch.float32 and not self.score32
        edge = VC_EDGE_TAIL if (replay and tail_columns(C) > 0) else VC_EDGE
        with on_device(dev):
            self._stats_all = torch.empty((sum(nbs), 2, D), dtype=torch.float64, device=dev)          # exchange 1
            self._csum_all = torch.zeros((W, 2 * Gmax, C), dtype=torch.float64, device=dev)           # exchange 2
            self._blocks_all = torch.zeros((W, int(vc_cap), 2 * edge + 1 + max(self.frames) * N // 16),
                                           dtype=torch.float32, device=dev)                           # exchange 2b
            self._s_all = torch.empty(self.F_total, dtype=torch.float32, device=dev)                  # exchange 3
            self._total = torch.empty(self.F_total * N, dtype=torch.float32, device=dev)
            chan = {"var_f32": torch.empty(D, dtype=torch.float32, device=dev),
                    "mask": torch.empty(D, dtype=torch.uint8, device=dev),
                    "cols": torch.empty(D, dtype=torch.int32, device=dev),
                    "perm": torch.empty(D, dtype=torch.int32, device=dev),
                    "spos": torch.empty(D, dtype=torch.int32, device=dev)}
            self.stages, b0 = [], 0
            for c, f in enumerate(self.frames):
                f0 = self.f0s[c]
                shared = dict(chan, stats=self._stats_all[b0: b0 + nbs[c]], csum=self._csum_all[c],
                              blocks=self._blocks_all[c], s=self._s_all[f0: f0 + f],
                              total=self._total[f0 * N: (f0 + f) * N])
                st = HipStages(f, N, D, dtype, dev, self.base, gather=False, vc_cap=vc_cap, frames=self.frames, rank=c,
                               params=self.params, score_dtype=score_dtype, shared=shared)
                st.F_total = self.F_total
                st.order_rider = c == 0                        # (the channel order is replayed once, by the first chunk's sweep 2)
                self.stages.append(st)
                b0 += nbs[c]
            # the selection's scratch (offsets, budgets) and the capacity of the unsharded pass for F_total frames
            n = ctypes.c_size_t(0)
            check(self._L.vc2_select_chunks_ws_bytes(self.F_total, ctypes.byref(n)), "vc2_select_chunks_ws_bytes")
            self._sel_ws = torch.empty(int(n.value), dtype=torch.uint8, device=dev)
        self.cap = min(self.F_total * N, int(self._L.vc2_kept_capacity(self.F_total, N, self.base)))
        self._chunk_rows = (ctypes.c_int64 * W)(*[f * N for f in self.frames])
        self._opts = self.stages[0]._opts
        self.arith_dtype = torch.float32 if self.score32 else dtype
        self.vc_fragile = 0

    # ---- the producer's side ----------------------------------------------------------------------------------------
    def _check_chunk(self, x, c: int) -> torch.Tensor:
        rows = self.frames[c] * self.N
        want_dev = self.device
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or tuple(x.shape) != (rows, self.D) or x.dtype != self.dtype \
                or x.device.type != want_dev.type or (want_dev.index is not None and x.device.index != want_dev.index):
            got = f"{x.dtype} {tuple(x.shape)} on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise RuntimeError(f"chunk {c} must be a {self.dtype} [{rows}, {self.D}] tensor on {want_dev} "
                               f"({self.frames[c]} frames of {self.N} tokens), got {got}")
        return x

    def add(self, chunk: torch.Tensor) -> None:
        """The next chunk, in frame order: its sweep 1 is enqueued at once; the last one enqueues the rest of the pass."""
        c = len(self._chunks)
        if c >= len(self.frames):
            raise RuntimeError(f"all {len(self.frames)} chunks of this video were added already: call finish() first")
        x = self._check_chunk(chunk, c)
        if self._hip:
            x = _vc._prep(x.detach(), f"chunk {c}")          # (contiguous, 16-byte aligned base: the sweeps load whole vectors)
            with on_device(self.device):
                self.stages[c].chan_stats(x)
                self._chunks.append(x)
                self._user_chunks.append(chunk)
                if c + 1 == len(self.frames):
                    self._enqueue_rest()
            return
        x = x if x.is_contiguous() else x.contiguous()
        self._stat_parts.append(self.stages[c].chan_stats(x))
        self._chunks.append(x)
        self._user_chunks.append(chunk)
        if c + 1 == len(self.frames):
            self._enqueue_rest()

    def _enqueue_rest(self) -> None:
        """Everything behind sweep 1, in the order of ShardedCompressor._enqueue; the exchanges are the shared buffers."""
        st, xs, hip = self.stages, self._chunks, self._hip
        R = self.F_total * self.N
        stats_all = self._stats_all if hip else torch.cat(self._stat_parts)
        for s in (st[:1] if hip else st):                      # (HIP: one selection, into the buffers all stages share)
            s.select_channels(stats_all, R)
        parts = [s.phase1(x) for s, x in zip(st, xs)]
        csum_all = self._csum_all if hip else torch.stack(parts)
        blocks = [s.vc_blocks(x, csum_all, R, f0) for s, x, f0 in zip(st, xs, self.f0s)] if hasattr(st[0], "vc_blocks") \
            else [None]
        gathered = (lambda bl: self._blocks_all) if hip else (lambda bl: torch.stack(list(bl)))
        if blocks[0] is not None and getattr(st[0], "needs_rounds", lambda: False)():
            n = st[0].flagged_columns()                        # (one host read: every stage holds the same count)
            for j0 in range(0, max(n, 1), st[0].vc_cap):
                if j0:
                    blocks = [s.vc_blocks_round(x, R, f0, j0) for s, x, f0 in zip(st, xs, self.f0s)]
                blocks_all = gathered(blocks)
                for s in st:
                    s.vc_finish_round(R, blocks_all, j0)
            s_parts = [s.phase2(x, csum_all, R, vc_final=True) for s, x in zip(st, xs)]
        elif blocks[0] is not None:
            blocks_all = gathered(blocks)
            s_parts = [s.phase2(x, csum_all, R, blocks_all) for s, x in zip(st, xs)]
        else:
            s_parts = [s.phase2(x, csum_all, R) for s, x in zip(st, xs)]
        if not hip:
            s_all = torch.cat([p.reshape(-1) for p in s_parts])
            for s, x, f0 in zip(st, xs, self.f0s):
                s.select(x, s_all, f0)
            self._pending = True
            return
        dev, D = self.device, self.D
        ks = torch.empty(self.F_total, dtype=torch.int64, device=dev)
        idx = torch.empty(self.cap, dtype=torch.int64, device=dev)
        kout = torch.zeros(4, dtype=torch.int64, device=dev)   # K, status bits, fragile centre columns, the gather's status
        rows = torch.empty((self.cap, D), dtype=self.dtype, device=dev) if self.gather else None
        table = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        s0 = st[0]
        args = (ptr(self._total), ptr(self._s_all), self.F_total, self.N, D, self.base, DTYPE_CODE[self.dtype],
                ptr(self._sel_ws), self._sel_ws.numel(), ptr(s0.ws), s0.ws.numel(), s0.F, ptr(ks), ptr(idx), self.cap,
                ptr(kout), table, self._chunk_rows, len(xs), ptr(rows), ctypes.c_void_p(kout.data_ptr() + 24),
                stream_ptr(dev))
        if self._opts is None:
            check(self._L.vc2_select_chunks(*args), "vc2_select_chunks")
        else:
            check(self._L.vc2_select_chunks_o(*args, ctypes.byref(self._opts)), "vc2_select_chunks_o")
        self._pending = (ks, idx, kout, rows)

    # ---- the consumer's side ----------------------------------------------------------------------------------------
    def finish(self) -> CompressionResult:
        if self._pending is None:
            raise RuntimeError(f"finish() after {len(self._chunks)} of {len(self.frames)} chunks: add the others first")
        pending, user = self._pending, self._user_chunks
        self.reset()                                           # ready for the next video
        if not self._hip:
            res = [s.result(f0) for s, f0 in zip(self.stages, self.f0s)]
            rows = torch.cat([r.rows for r in res]) if self.gather else None
            return CompressionResult(rows, torch.cat([r.global_idx for r in res]), torch.cat([r.ks for r in res]),
                                     sum(r.K for r in res))
        ks, idx, kout, rows = pending
        grad = self.gather and _ag.wants_grad(*user)
        if grad:                                               # (the chunks' kept counts ride along in the one read)
            words = torch.cat([kout, ks.clamp(max=self.N)]).tolist()
        else:
            words = kout.tolist()                              # the pass's single host sync
        K, status, fragile, gstatus = (int(w) for w in words[:4])
        if status:
            _vc._raise_status(status, self.cap, K)
        if gstatus & 0xFFFFFFFF:
            raise RuntimeError(f"vidcom2_amd: the chunk gather skipped a row (status {gstatus & 0xFFFFFFFF:#x}: an index "
                               "outside the video or the output) -- please report")
        self.vc_fragile = fragile
        if fragile and _ffi.get_mode() == "torch":
            warnings.warn(f"vidcom2_amd (frame-sharded pass): {fragile} video-centre value(s) lie within the replay margin "
                          "of a rounding boundary and could not be replayed across ranks "
                          f"(more than {self.stages[0].vc_cap} such columns in a mode that does not go in rounds); they keep "
                          "the exactly rounded mean, the reference's fp32 summation order could round the other way.",
                          RuntimeWarning, stacklevel=2)
        res = CompressionResult(rows[:K] if rows is not None else None, idx[:K], ks, K)
        _vc._check_budgets(ks, self.N, self.arith_dtype)
        if grad:
            per_frame = words[4:]
            counts = [sum(per_frame[f0: f0 + f]) for f0, f in zip(self.f0s, self.frames)]
            spec = (res.global_idx, counts, self.starts, [tuple(u.shape) for u in user])
            res.rows = _GatherChunks.apply(_ag._Box(res.rows.detach(), spec), *user)
        return res

    def reset(self) -> None:
        """Forget the chunks added so far (a video that was abandoned half way)."""
        self._chunks, self._user_chunks, self._stat_parts, self._pending = [], [], [], None

    def __call__(self, chunks) -> CompressionResult:
        if len(chunks) != len(self.frames):
            raise RuntimeError(f"{len(chunks)} chunks for a layout of {len(self.frames)}")
        for c, x in enumerate(chunks):                        # (everything is checked before anything is enqueued)
            self._check_chunk(x, c)
        self.reset()
        for x in chunks:
            self.add(x)
        return self.finish()


_CACHE: "OrderedDict" = OrderedDict()
_CACHE_MAX = 2


def clear_chunk_cache() -> None:
    """Drop the compressors (workspaces and whole-video buffers) compress_chunks keeps for the last layouts it saw."""
    _CACHE.clear()


def compress_chunks(chunks, tpf: int, base_scale: float = 0.25, gather: bool = True, params=None, score_dtype=None,
                    stages_factory: Optional[Callable] = None) -> CompressionResult:
    """`compress(torch.cat(chunks), tpf, base_scale, gather=gather, params=params, score_dtype=score_dtype)` for the linear
    mapper without the concatenation: chunks is a list of [F_c * tpf, D] tensors of one dtype, device and D, at least one
    frame each, in frame order (at most 64; frame counts may differ).  global_idx indexes the virtual torch.cat(chunks) and
    rows == torch.cat(chunks)[global_idx] ([K, D], None with gather=False; differentiable with respect to every chunk, as
    in `compress`).  One chunk delegates to `compress`.  Numerics and limits: see the module docstring.  The compressors
    of the last two layouts are kept (clear_chunk_cache)."""
    chunks = list(chunks)
    if not chunks:
        raise ValueError("compress_chunks needs at least one chunk (got an empty list)")
    if len(chunks) > MAX_CHUNKS:
        raise NotImplementedError(f"{len(chunks)} chunks: at most {MAX_CHUNKS} are supported (concatenate neighbours)")
    tpf = int(tpf)
    x0 = chunks[0]
    if not isinstance(x0, torch.Tensor) or x0.dim() != 2:
        raise RuntimeError(f"every chunk must be a 2-D [frames*tokens, dim] tensor, got "
                           f"{tuple(x0.shape) if isinstance(x0, torch.Tensor) else type(x0).__name__}")
    D, dtype, device = int(x0.shape[1]), x0.dtype, x0.device
    params_n = _vc._norm_params(params)
    _vc._norm_score_dtype(score_dtype, dtype)
    _vc._c_params(params_n, D)
    frames = []
    for c, x in enumerate(chunks):
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.shape[1] != D or x.dtype != dtype or x.device != device:
            got = f"{x.dtype} {tuple(x.shape)} on {x.device}" if isinstance(x, torch.Tensor) else type(x).__name__
            raise RuntimeError(f"chunk {c} must be a {dtype} [frames * {tpf}, {D}] tensor on {device}, got {got}")
        R = int(x.shape[0])
        if tpf <= 0 or R == 0 or R % tpf != 0:
            # the reference fails in frames = x.view(-1, tpf, C) (vidcom2.py:47); here a chunk must hold whole frames
            C = int(D * 0.5) if params_n is None else params_n.channels(D)
            raise RuntimeError(f"shape '[-1, {tpf}, {C}]' is invalid for input of size {R * C}")
        frames.append(R // tpf)
    if len(chunks) == 1 and stages_factory is None:
        return _vc.compress(x0, tpf, base_scale, gather=gather, params=params, score_dtype=score_dtype)
    if stages_factory is not None:
        return ChunkedCompressor(frames, tpf, D, dtype, device, base_scale, gather, params, score_dtype,
                                 stages_factory=stages_factory)(chunks)
    require_device(x0, "chunks")
    key = (tuple(frames), tpf, D, dtype, device, float(base_scale), bool(gather), params_n,
           _vc._norm_score_dtype(score_dtype, dtype), _ffi.lib().vc2_get_mode())
    cc = _CACHE.get(key)
    if cc is None:
        cc = ChunkedCompressor(frames, tpf, D, dtype, device, base_scale, gather, params, score_dtype)
        _CACHE[key] = cc
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
    else:
        _CACHE.move_to_end(key)
    return cc(chunks)

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

The options the LLaVA hooks hand to `compress` are taken here too (keyword-only, all off by default -- the calls above are
then issued exactly as without them): `mapper="grid_vid"` / `grid_h` / `newline` (LLaVA-Video: indices in the slot space
of the [F_total * h * (h + 1), D] stream, newline rows written from the vector), `tail` (OneVision's newline row behind the
kept ones), `want_scores` (whole-video v_score / f_score) -- selection and gather are then `vc2_select_chunks_x` and
`k_gather_rows_grid_chunks` -- and `ChunkedCompressor.add_pooled`, which pools a chunk 2x2 and takes its channel
statistics from the pooling sweep (`vc2_pool_stats_blocks`) instead of a sweep 1.

Numerics (the sharded pass's own contract): chunks that are each a multiple of 16 frames give the bits of
`compress(torch.cat(chunks))`.  Other splits give the same channel variances and centre sums up to fp64 rounding before
they are rounded to T; the video-centre replay then goes through the ragged exchange-2b forms.  Leftover fragile
video-centre columns are reported by the same RuntimeWarning as `HipStages.result`.  At most 64 chunks
(VC2_RAGGED_MAX_WORLD).

Not offered here: an `img_feat` form of the grid mapping (chunks are gathered from directly: give `newline`), these
options in the multi-GPU `ShardedCompressor`, chunks on different devices.
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
from ._ffi import DTYPE_CODE, MAP_GRID_VID, MAP_LINEAR, check, lib, on_device, ptr, require_device, stream_ptr
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


def _check_mapping(mapper, grid_h, newline, N: int) -> int:
    """`compress`'s argument errors for the mapper, before anything else is looked at; returns the grid height (0: linear)."""
    if newline is not None and mapper != "grid_vid":
        raise ValueError(f"newline is the grid_vid mapper's newline vector; got mapper={mapper!r}")
    if mapper not in ("linear", "grid_vid"):
        raise ValueError(f"unknown mapper {mapper!r}")
    if mapper == "linear":
        return 0
    if newline is None:                                     # (chunks offer no img_feat form)
        raise ValueError("img_feat required for grid mapping")
    h = int(grid_h)
    if h <= 0 or h * h != int(N):                           # (what vc2_compress_ex5 answers, raised by `check`)
        raise RuntimeError("vc2_compress failed (code -1): grid_vid mapping needs N == grid_h^2")
    return h


def _prep_tail(tail, D: int, dtype, device) -> Optional[torch.Tensor]:
    """`compress`'s tail ([m, D] or [D], the chunks' dtype and device) as the contiguous [m, D] tensor the gather reads."""
    if tail is None:
        return None
    device = torch.device(device)
    ok = isinstance(tail, torch.Tensor) and tail.dim() in (1, 2) and tail.shape[-1] == D and tail.dtype == dtype \
        and tail.device.type == device.type and (device.index is None or tail.device.index == device.index)
    if not ok:
        got = f"{tuple(tail.shape)} {tail.dtype} on {tail.device}" if isinstance(tail, torch.Tensor) else type(tail).__name__
        raise RuntimeError(f"tail must be [m, {D}] {dtype} on {device}, got {got}")
    tail = tail.detach()
    tail = tail if tail.dim() == 2 else tail[None]
    return tail if tail.is_contiguous() else tail.contiguous()


def _grid_slots(global_idx: torch.Tensor, ks: torch.Tensor, N: int, h: int) -> torch.Tensor:
    """vidcom2.py:105-115 in plain torch on the linear indices of the virtual concatenation (frame by frame, in the order
    the selection left them): every frame's kept tokens on the h x (h + 1) grid, then its h newline slots."""
    w, out, k0 = h + 1, [], 0
    for f, k in enumerate(ks.clamp(max=N).tolist()):
        loc = global_idx[k0: k0 + k] - f * N
        out.append(f * h * w + (loc // h) * w + loc % h)
        out.append(f * h * w + torch.arange(h, dtype=torch.int64, device=global_idx.device) * w + h)
        k0 += k
    return torch.cat(out)


class _GatherChunksX(torch.autograd.Function):
    """rows of the chunk gather with options (k_gather_rows_grid_chunks): kept rows of the chunks, newline rows (grid
    mapping), tail rows.  The backward is composed from what exists, like autograd._GatherRowsGrid: every chunk gets the
    rows of the output gradient that came from it through vc2_rows_grad (its sub-range of the index list in the chunk's own
    rows, newline slots as -1 entries, which it skips), the newline slots' gradient rows are summed in fp32 and rounded once,
    the tail is the last m rows."""

    @staticmethod
    def forward(ctx, box, newline, tail, *chunks):
        ctx.spec = box.spec
        return box.outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        idx, K, counts, starts, shapes, h, nl_shape, tail_shape = ctx.spec
        D = int(g.shape[-1])
        g = g.reshape(-1, D)
        g = g if g.is_contiguous() else g.contiguous()
        gi = idx[:K]
        if h:                                                  # slot -> row of the virtual concatenation, -1 for a newline
            w = h + 1
            c = gi % w
            is_nl = c == h
            gi = torch.where(is_nl, torch.full_like(gi, -1), (gi // (h * w)) * (h * h) + ((gi % (h * w)) // w) * h + c)
        out, k0 = [], 0
        for ci, n in enumerate(counts):
            rows_c = starts[ci + 1] - starts[ci]
            if not ctx.needs_input_grad[3 + ci]:
                out.append(None)
            elif n == 0:
                out.append(torch.zeros(shapes[ci], dtype=g.dtype, device=g.device))
            else:
                part = gi[k0: k0 + n]
                local = torch.where(part < 0, part, part - starts[ci]).contiguous() if h else part - starts[ci]
                out.append(_ag.rows_grad([g], [rows_c], local, n, dst_row0=k0)[0].view(shapes[ci]))
            k0 += n
        gnl = gtail = None
        if h and ctx.needs_input_grad[1]:
            gnl = g[:K][is_nl].float().sum(dim=0).to(g.dtype).reshape(nl_shape)
        if tail_shape is not None and ctx.needs_input_grad[2]:
            gtail = g[K: K + int(torch.Size(tail_shape[:-1]).numel())].reshape(tail_shape)
        return (None, gnl, gtail) + tuple(out)


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
    inject CPU stages): the driver then exchanges by torch.cat / torch.stack and selects per chunk, and honours the options
    below with plain torch indexing on the concatenation (with want_scores the stage objects must leave their [F_c, N]
    scores in `.v` / `.f` after phase2).  None: the HIP stages on shared whole-video buffers, `vc2_select_chunks` and the
    chunk gather.

    mapper / grid_h / newline / tail / want_scores (keyword-only): as in `compress` -- the result is that of
    `compress(torch.cat(chunks), N, base_scale, mapper, grid_h, newline=, tail=, want_scores=, ...)`: with "grid_vid",
    global_idx is in the slot space of the [F_total * h * (h + 1), D] stream and K counts the newline rows; with a tail of
    m rows, rows is [K + m, D]; with want_scores, v_score / f_score are [F_total, N] in the dtype the pass scores in.  The
    newline and tail TENSORS may be replaced per video (`cc(chunks, newline=, tail=)`, same shapes).  rows is
    differentiable with respect to every chunk, newline and tail.
    """

    def __init__(self, frames, N: int, D: int, dtype, device, base_scale: float = 0.25, gather: bool = True,
                 params=None, score_dtype=None, stages_factory: Optional[Callable] = None, vc_cap: int = 64, *,
                 mapper: str = "linear", grid_h: int = 0, newline=None, tail=None, want_scores: bool = False):
        self.grid_h = _check_mapping(mapper, grid_h, newline, N)       # (argument errors first, as in `compress`)
        self.frames = _check_layout(frames)
        self.N, self.D, self.dtype, self.device = int(N), int(D), dtype, torch.device(device)
        self.base, self.gather = float(base_scale), bool(gather)
        self.want_scores = bool(want_scores)
        self._set_row_inputs(newline, tail, first=True)
        # bad params / score_dtype: exactly what HipStages raises, before a stage exists
        self.params = _vc._norm_params(params)
        self.score32 = _vc._norm_score_dtype(score_dtype, dtype) is not None
        cparams = _vc._c_params(self.params, self.D)
        W = len(self.frames)
        self.F_total = sum(self.frames)
        self.f0s = [sum(self.frames[:c]) for c in range(W)]
        self.starts = chunk_starts([f * self.N for f in self.frames])
        self._hip = stages_factory is None
        self._v_all = self._f_all = None
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
            self._new_scores()                                                                        # (want_scores only)
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
                if self.want_scores:
                    shared.update(v=self._v_all[f0: f0 + f], f=self._f_all[f0: f0 + f])
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
        self.cap += self.F_total * self.grid_h                 # (every frame's newline slots, as CompressPlan counts them)
        self._chunk_rows = (ctypes.c_int64 * W)(*[f * N for f in self.frames])
        self._opts = self.stages[0]._opts
        self.arith_dtype = torch.float32 if self.score32 else dtype
        self.vc_fragile = 0

    def _set_row_inputs(self, newline, tail, first: bool = False) -> None:
        """This video's newline vector and tail rows (`_prep_newline`'s / `compress`'s errors); later videos may bring other
        tensors of the same shapes."""
        nl = _vc._prep_newline(newline, self.D, self.dtype, self.device) if newline is not None else None
        tl = _prep_tail(tail, self.D, self.dtype, self.device) if self.gather else None
        if not first:
            if (nl is None) != (self._newline is None):
                raise ValueError("newline is the grid_vid mapper's newline vector: a compressor is built with or without one")
            if (0 if tl is None else tl.shape[0]) != self.tail_rows:
                raise RuntimeError(f"tail must be [{self.tail_rows}, {self.D}] {self.dtype} on {self.device}")
        self._newline, self._tail = nl, tl
        self._newline_user, self._tail_user = newline, (tail if self.gather else None)
        self.tail_rows = 0 if tl is None else int(tl.shape[0])

    def _new_scores(self) -> None:
        """Fresh whole-video score tensors for the next video (a result handed out earlier is never overwritten)."""
        if self.want_scores and self._v_all is None:
            sdt = torch.float32 if self.score32 else self.dtype
            self._v_all = torch.empty((self.F_total, self.N), dtype=sdt, device=self.device)
            self._f_all = torch.empty((self.F_total, self.N), dtype=sdt, device=self.device)

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

    def add_pooled(self, image_feature: torch.Tensor, height: int, width: int, mode: str = "average") -> torch.Tensor:
        """The next chunk as the projector's output [F_c, height * width, D]: pooled 2x2 (`fused.pool_stats`'s modes, limits
        and bits) into a fresh [F_c, h * w, D] tensor by the sweep that also takes its channel statistics
        (vc2_pool_stats_blocks: the chunk's slot of the exchange-1 buffer holds what `add` would have written), so the
        chunk is added without a sweep 1.  h * w must be N.  Returns the pooled tensor (a plain tensor: autograd through
        the pooling is the caller's `autograd.attach_pool`).  May be mixed with `add` within one video."""
        from .fused import POOL_MODES
        require_device(image_feature, "image_feature")
        if mode not in POOL_MODES:
            raise ValueError(f"Unexpected mm_spatial_pool_mode: {mode}")
        if not self._hip:
            raise RuntimeError("add_pooled runs the pooling sweep of the HIP stages: injected stages take add(chunk)")
        c = len(self._chunks)
        if c >= len(self.frames):
            raise RuntimeError(f"all {len(self.frames)} chunks of this video were added already: call finish() first")
        x, H, W = image_feature, int(height), int(width)
        if x.dim() != 3 or x.shape[1] != H * W:
            raise RuntimeError(f"image_feature must be [frames, {height}*{width}, dim], got {tuple(x.shape)}")
        h, w = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self._L.vc2_pool_out_tokens(H, W, POOL_MODES[mode], ctypes.byref(h), ctypes.byref(w)), "vc2_pool_out_tokens")
        n = int(h.value) * int(w.value)
        dev = self.device
        if n != self.N or tuple(x.shape) != (self.frames[c], H * W, self.D) or x.dtype != self.dtype \
                or (dev.index is not None and x.device.index != dev.index):
            raise RuntimeError(f"chunk {c} must pool to a {self.dtype} [{self.frames[c]}, {self.N}, {self.D}] tensor on "
                               f"{dev}, got {x.dtype} {tuple(x.shape)} on {x.device} pooling to {n} tokens per frame")
        x = _vc._prep(x.detach(), f"chunk {c}")
        st = self.stages[c]
        with on_device(dev):
            out = torch.empty((self.frames[c], n, self.D), dtype=self.dtype, device=dev)
            check(self._L.vc2_pool_stats_blocks(ptr(x), st.F, H, W, self.D, st.code, POOL_MODES[mode], self.F_total, st.bf,
                                                ptr(st.ws), st.ws.numel(), ptr(out), ptr(st.stats), stream_ptr(dev),
                                                ctypes.byref(st._opts) if st._opts is not None else None),
                  "vc2_pool_stats_blocks")
            flat = out.view(self.frames[c] * n, self.D)
            self._chunks.append(flat)
            self._user_chunks.append(flat)
            if c + 1 == len(self.frames):
                self._enqueue_rest()
        return out

    def _enqueue_rest(self) -> None:
        """Everything behind sweep 1, in the order of ShardedCompressor._enqueue; the exchanges are the shared buffers."""
        st, xs, hip = self.stages, self._chunks, self._hip
        R = self.F_total * self.N
        if hip and self.want_scores and self._v_all is None:   # (the last video took the score tensors: fresh ones)
            self._new_scores()
            for s, f0 in zip(st, self.f0s):
                s.set_score_views(self._v_all[f0: f0 + s.F], self._f_all[f0: f0 + s.F])
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
            if self.want_scores:                               # (stage objects leave their [F_c, N] scores in .v / .f)
                self._v_all, self._f_all = (torch.cat([getattr(s, n).reshape(s.F, self.N) for s in st]) for n in "vf")
            self._pending = True
            return
        dev, D = self.device, self.D
        ks = torch.empty(self.F_total, dtype=torch.int64, device=dev)
        idx = torch.empty(self.cap, dtype=torch.int64, device=dev)
        kout = torch.zeros(4, dtype=torch.int64, device=dev)   # K, status bits, fragile centre columns, the gather's status
        rows = torch.empty((self.cap + self.tail_rows, D), dtype=self.dtype, device=dev) if self.gather else None
        table = (ctypes.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
        s0 = st[0]
        args = (ptr(self._total), ptr(self._s_all), self.F_total, self.N, D, self.base, DTYPE_CODE[self.dtype],
                ptr(self._sel_ws), self._sel_ws.numel(), ptr(s0.ws), s0.ws.numel(), s0.F, ptr(ks), ptr(idx), self.cap,
                ptr(kout), table, self._chunk_rows, len(xs), ptr(rows), ctypes.c_void_p(kout.data_ptr() + 24),
                stream_ptr(dev))
        if self.grid_h or self.tail_rows:                      # (the mapping and gather options: their own entry point)
            check(self._L.vc2_select_chunks_x(*args, ctypes.byref(self._opts) if self._opts is not None else None,
                                              MAP_GRID_VID if self.grid_h else MAP_LINEAR, self.grid_h,
                                              ptr(self._newline), ptr(self._tail), self.tail_rows), "vc2_select_chunks_x")
        elif self._opts is None:
            check(self._L.vc2_select_chunks(*args), "vc2_select_chunks")
        else:
            check(self._L.vc2_select_chunks_o(*args, ctypes.byref(self._opts)), "vc2_select_chunks_o")
        self._pending = (ks, idx, kout, rows)

    # ---- the consumer's side ----------------------------------------------------------------------------------------
    def finish(self) -> CompressionResult:
        if self._pending is None:
            raise RuntimeError(f"finish() after {len(self._chunks)} of {len(self.frames)} chunks: add the others first")
        pending, user = self._pending, self._user_chunks
        v_all, f_all, self._v_all, self._f_all = self._v_all, self._f_all, None, None
        self.reset()                                           # ready for the next video
        if not self._hip:
            # the executable definition of the options: plain torch indexing on the concatenation
            res = [s.result(f0) for s, f0 in zip(self.stages, self.f0s)]
            gidx, ks = torch.cat([r.global_idx for r in res]), torch.cat([r.ks for r in res])
            rows = torch.cat([r.rows for r in res]) if self.gather else None
            if self.grid_h:
                h = self.grid_h
                gidx = _grid_slots(gidx, ks, self.N, h)
                if self.gather:
                    stream = torch.cat([torch.cat(user).view(self.F_total, h, h, self.D),
                                        self._newline.view(1, 1, 1, self.D).expand(self.F_total, h, 1, self.D)], dim=2)
                    rows = stream.reshape(-1, self.D)[gidx]
            if self._tail is not None:
                rows = torch.cat([rows, self._tail])
            return CompressionResult(rows, gidx, ks, int(gidx.numel()), v_all, f_all)
        ks, idx, kout, rows = pending
        nl_user, tail_user, h, m = self._newline_user, self._tail_user, self.grid_h, self.tail_rows
        grad = self.gather and _ag.wants_grad(*user, nl_user, tail_user)
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
        res = CompressionResult(rows[:K + m] if rows is not None else None, idx[:K], ks, K, v_all, f_all)
        _vc._check_budgets(ks, self.N, self.arith_dtype)
        if grad:                                               # (grid: every frame's h newline slots follow its kept tokens)
            per_frame = words[4:]
            counts = [sum(per_frame[f0: f0 + f]) + f * h for f0, f in zip(self.f0s, self.frames)]
            shapes = [tuple(u.shape) for u in user]
            if h or m:
                spec = (res.global_idx, K, counts, self.starts, shapes, h,
                        tuple(nl_user.shape) if nl_user is not None else None,
                        tuple(tail_user.shape) if tail_user is not None else None)
                res.rows = _GatherChunksX.apply(_ag._Box(res.rows.detach(), spec), nl_user, tail_user, *user)
            else:
                res.rows = _GatherChunks.apply(_ag._Box(res.rows.detach(), (res.global_idx, counts, self.starts, shapes)),
                                               *user)
        return res

    def reset(self) -> None:
        """Forget the chunks added so far (a video that was abandoned half way)."""
        self._chunks, self._user_chunks, self._stat_parts, self._pending = [], [], [], None

    def __call__(self, chunks, *, newline=None, tail=None) -> CompressionResult:
        """One video at once.  newline / tail: this video's tensors in place of the ones the compressor was built with
        (same shapes; a compressor built without one takes none)."""
        if len(chunks) != len(self.frames):
            raise RuntimeError(f"{len(chunks)} chunks for a layout of {len(self.frames)}")
        for c, x in enumerate(chunks):                        # (everything is checked before anything is enqueued)
            self._check_chunk(x, c)
        if newline is not None or tail is not None:
            self._set_row_inputs(newline if newline is not None else self._newline_user,
                                 tail if tail is not None else self._tail_user)
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
                    stages_factory: Optional[Callable] = None, *, mapper: str = "linear", grid_h: int = 0, newline=None,
                    tail=None, want_scores: bool = False) -> CompressionResult:
    """`compress(torch.cat(chunks), tpf, base_scale, mapper, grid_h, newline=newline, tail=tail, want_scores=want_scores,
    gather=gather, params=params, score_dtype=score_dtype)` without the concatenation: chunks is a list of [F_c * tpf, D]
    tensors of one dtype, device and D, at least one frame each, in frame order (at most 64; frame counts may differ).
    Linear mapper: global_idx indexes the virtual torch.cat(chunks) and rows == torch.cat(chunks)[global_idx].  "grid_vid"
    with `newline` (there is no img_feat form): global_idx indexes the [F_total * h * (h + 1), D] stream add_token_per_grid
    would build from torch.cat(chunks) and the newline vector, K counts the newline rows, and neither is built.  tail
    ([m, D]): rows is [K + m, D].  want_scores: v_score / f_score [F_total, N].  rows is None with gather=False (indices are
    still mapped) and differentiable with respect to every chunk, newline and tail, as in `compress`.  One chunk delegates to
    `compress`.  Numerics and limits: see the module docstring.  The compressors of the last two layouts are kept
    (clear_chunk_cache); the newline and tail tensors are each call's own."""
    _check_mapping(mapper, grid_h, newline, int(tpf))          # (argument errors first, as in `compress`)
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
    if newline is not None:
        _vc._prep_newline(newline, D, dtype, device)
    tail_n = _prep_tail(tail, D, dtype, device)
    plain = mapper == "linear" and tail is None and not want_scores
    opts = {} if plain else dict(mapper=mapper, grid_h=grid_h, newline=newline, tail=tail, want_scores=want_scores)
    if len(chunks) == 1 and stages_factory is None:
        return _vc.compress(x0, tpf, base_scale, gather=gather, params=params, score_dtype=score_dtype, **opts)
    if stages_factory is not None:
        return ChunkedCompressor(frames, tpf, D, dtype, device, base_scale, gather, params, score_dtype,
                                 stages_factory=stages_factory, **opts)(chunks)
    require_device(x0, "chunks")
    key = (tuple(frames), tpf, D, dtype, device, float(base_scale), bool(gather), params_n,
           _vc._norm_score_dtype(score_dtype, dtype), _ffi.lib().vc2_get_mode())
    if not plain:                                              # (the tensors themselves are per call)
        key += (mapper, int(grid_h), newline is not None, 0 if tail_n is None else int(tail_n.shape[0]), bool(want_scores))
    cc = _CACHE.get(key)
    if cc is None:
        cc = ChunkedCompressor(frames, tpf, D, dtype, device, base_scale, gather, params, score_dtype, **opts)
        _CACHE[key] = cc
        while len(_CACHE) > _CACHE_MAX:
            _CACHE.popitem(last=False)
        return cc(chunks)
    _CACHE.move_to_end(key)
    return cc(chunks, newline=newline, tail=tail)

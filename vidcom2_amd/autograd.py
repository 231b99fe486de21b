"""Backward of the kept-row / kept-column gathers, so that training runs see the gradients the reference's plain
torch indexing gives (vidcom2.py:43,91,96; the hooks' torch.cat / inputs_embeds[:, keep]).

Every differentiable output is produced by the same forward launches as without autograd; a `torch.autograd.Function`
is attached to it only when `torch.is_grad_enabled()` and a floating input requires grad (`wants_grad`), so under
`torch.no_grad()` / `torch.inference_mode()` and for inputs that do not require grad nothing changes.  The Functions
save the index list, the counts and the shapes -- never the gathered-from tensor, like torch's own backward of
`flat[idx]` -- and their backward is one HIP pass that writes every input-gradient row once (`vc2_rows_grad`,
`vc2_cols_grad`, include/vc2.h), bit-identical to torch's `zeros_like(x).index_put_(idx, g, accumulate=True)`.
Not differentiable: the scores (`compute_gaussian_scores`, `_multi_scale_gaussian`, `compute_scales`, `want_scores`),
indices and budgets, `CompressPlan` used directly, `sharded.py`, and `fused.gather_scatter` / `fused.repad_rows`
writing into caller-provided destinations.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Sequence

import torch
from torch.autograd.function import once_differentiable

from ._ffi import DTYPE_CODE, check, lib, on_device, ptr, stream_ptr

__all__ = ["wants_grad", "rows_grad", "cols_grad", "attach_rows", "attach_rows_grid", "attach_cols", "attach_pool"]


def wants_grad(*ts) -> bool:
    """Is an autograd graph being recorded and does a floating input require grad?"""
    return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad and t.is_floating_point()
                                           for t in ts)


def _ptrs(ts: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _i64s(vs: Sequence[int]):
    return (ctypes.c_int64 * len(vs))(*[int(v) for v in vs])


def rows_grad(gdsts: Sequence[Optional[torch.Tensor]], src_rows: Sequence[int], idx: Optional[torch.Tensor], n: int,
              n_dev: Optional[torch.Tensor] = None, dst_row0: int = 0,
              validate: bool = False) -> List[Optional[torch.Tensor]]:
    """Gradients [src_rows[t], D] of row gathers dst_t[dst_row0 + j] = src_t[idx[j] or j] (j < n; n_dev caps n on the
    device) from the output gradients gdsts[t] ([rows, D]; None: that source gets None).  validate: read the status
    word back and, on a duplicate or out-of-range index, redo the backward with torch's accumulating scatter (for index
    lists the caller supplied; the lists the library builds itself are unique by construction and skip the read-back)."""
    live = [t for t, g in enumerate(gdsts) if g is not None]
    out: List[Optional[torch.Tensor]] = [None] * len(gdsts)
    if not live:
        return out
    gd = [gdsts[t] if gdsts[t].is_contiguous() else gdsts[t].contiguous() for t in live]
    g0 = gd[0]
    D = int(g0.shape[1])
    dev = g0.device
    res = [torch.empty((int(src_rows[t]), D), dtype=g0.dtype, device=dev) for t in live]
    rows_max = max(int(src_rows[t]) for t in live)
    inv = torch.empty(max(rows_max, 1), dtype=torch.int32, device=dev) if idx is not None else None
    status = torch.zeros(1, dtype=torch.int32, device=dev) if validate else None
    with on_device(dev):
        rc = lib().vc2_rows_grad(_ptrs(gd), _i64s([g.shape[0] for g in gd]), _ptrs(res), _i64s([r.shape[0] for r in res]),
                                 len(live), D, DTYPE_CODE[g0.dtype], ptr(idx), ptr(n_dev), int(n), int(dst_row0), ptr(inv),
                                 inv.numel() if inv is not None else 0, ptr(status), stream_ptr(dev))
    check(rc, "vc2_rows_grad")
    if validate and int(status.item()):
        # a duplicate (or out-of-range) index: torch's own accumulating scatter, which also raises on the latter
        nn = int(n) if n_dev is None else min(int(n_dev.reshape(-1)[0].item()), int(n))
        ii = idx[:nn]
        sel = ii >= 0
        res = [torch.zeros_like(r).index_put_((ii[sel],), g[dst_row0:dst_row0 + nn][sel], accumulate=True)
               for r, g in zip(res, gd)]
    for t, r in zip(live, res):
        out[t] = r
    return out


def cols_grad(g: torch.Tensor, idx: torch.Tensor, D: int) -> torch.Tensor:
    """Gradient [R, D] of out = x[:, idx] (idx: C unique columns) from g [R, C]."""
    g = g if g.is_contiguous() else g.contiguous()
    R, C = (int(v) for v in g.shape)
    gx = torch.empty((R, int(D)), dtype=g.dtype, device=g.device)
    with on_device(g.device):
        rc = lib().vc2_cols_grad(ptr(g), R, C, int(D), DTYPE_CODE[g.dtype], ptr(idx), ptr(gx), None, stream_ptr(g.device))
    check(rc, "vc2_cols_grad")
    return gx


class _Box:
    """Non-tensor argument of the Functions below: the forward's results (made by the HIP launches before `apply`)
    and what the backward needs."""
    __slots__ = ("outs", "spec")

    def __init__(self, outs, spec):
        self.outs, self.spec = outs, spec


class _RowsSpec:
    __slots__ = ("idx", "n", "n_dev", "dst_row0", "src_shapes", "rows_d", "tail_shape", "validate")

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)


class _GatherRows(torch.autograd.Function):
    """outs[t] = rows of srcs[t] gathered by one index list; outs[0] may carry `tail` rows behind the gathered ones."""

    @staticmethod
    def forward(ctx, box, *inputs):                      # inputs = srcs..., tail (or None)
        ctx.spec = box.spec
        return tuple(box.outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        sp: _RowsSpec = ctx.spec
        ns = len(sp.src_shapes)
        need = ctx.needs_input_grad[1:]
        D = [d for _, d in sp.rows_d]
        gd = [g.reshape(-1, D[t]) if (need[t] and g is not None) else None for t, g in enumerate(grads)]
        gs = rows_grad(gd, [r for r, _ in sp.rows_d], sp.idx, sp.n, sp.n_dev, sp.dst_row0, sp.validate)
        gs = [g.view(sp.src_shapes[t]) if g is not None else None for t, g in enumerate(gs)]
        gtail = None
        if sp.tail_shape is not None and need[ns] and grads[0] is not None:
            m = int(torch.Size(sp.tail_shape[:-1]).numel())
            g0 = grads[0].reshape(-1, D[0])
            if sp.n_dev is None:
                gtail = g0[sp.dst_row0 + sp.n: sp.dst_row0 + sp.n + m]
            else:                                        # (n known on the device only: the tail sits behind row n)
                first = torch.clamp(sp.n_dev.reshape(-1)[:1], max=sp.n) + sp.dst_row0
                gtail = g0.index_select(0, first + torch.arange(m, device=g0.device))
            gtail = gtail.reshape(sp.tail_shape)
        return (None,) + tuple(gs) + (gtail,)


def attach_rows(outs: Sequence[torch.Tensor], srcs: Sequence[torch.Tensor], idx: Optional[torch.Tensor], n: int,
                tail: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None, dst_row0: int = 0,
                validate: bool = False, row_len: Optional[int] = None) -> List[torch.Tensor]:
    """The already gathered `outs` (outs[t] from srcs[t], rows dst_row0 + j <- idx[j]; tail rows behind them in outs[0])
    returned as outputs of a differentiable gather: same tensors' storage, a grad_fn attached.  A source is viewed as
    rows of `row_len` elements (default: everything behind its first dimension)."""
    shapes = [tuple(s.shape) for s in srcs]
    rows_d = [(s.numel() // row_len, row_len) if row_len else (sh[0], int(torch.Size(sh[1:]).numel()))
              for s, sh in zip(srcs, shapes)]
    spec = _RowsSpec(idx=idx, n=int(n), n_dev=n_dev, dst_row0=int(dst_row0), src_shapes=shapes, rows_d=rows_d,
                     tail_shape=tuple(tail.shape) if tail is not None else None, validate=bool(validate))
    # (detach: an output that is a view -- the kept rows sliced from a plan's buffer -- would refuse in-place use)
    return list(_GatherRows.apply(_Box([o.detach() for o in outs], spec), *srcs, tail))


class _GatherRowsGrid(torch.autograd.Function):
    """out = rows of the [F*h*(h+1), D] stream made of `flat` [F*h*h, D] and the [D] newline vector (the grid form of the
    gather, vc2_gather_rows_grid), gathered by grid-space indices; `tail` rows may sit behind them.  The backward is
    composed from what exists: the non-newline slots go through vc2_rows_grad (the newline slots become pad entries, -1,
    which it skips), the newline slots' gradient rows are summed in fp32 and rounded once."""

    @staticmethod
    def forward(ctx, box, flat, newline, tail):
        ctx.spec = box.spec
        return box.outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        idx, n, F, h, flat_shape, nl_shape, tail_shape, validate = ctx.spec
        need_flat, need_nl, need_tail = ctx.needs_input_grad[1:4]
        D = int(g.shape[-1])
        g = g.reshape(-1, D)
        g = g if g.is_contiguous() else g.contiguous()
        gi = idx[:n]
        w = h + 1
        c = gi % w
        is_nl = c == h
        gflat = gnl = gtail = None
        if need_flat:
            src = torch.where(is_nl, torch.full_like(gi, -1), (gi // (h * w)) * (h * h) + ((gi % (h * w)) // w) * h + c)
            gflat = rows_grad([g], [F * h * h], src.contiguous(), n, validate=validate)[0].view(flat_shape)
        if need_nl:
            gnl = g[:n][is_nl].float().sum(dim=0).to(g.dtype).reshape(nl_shape)
        if need_tail and tail_shape is not None:
            gtail = g[n: n + int(torch.Size(tail_shape[:-1]).numel())].reshape(tail_shape)
        return None, gflat, gnl, gtail


def attach_rows_grid(out: torch.Tensor, flat: torch.Tensor, newline: torch.Tensor, idx: torch.Tensor, n: int, F: int,
                     h: int, tail: Optional[torch.Tensor] = None, validate: bool = False) -> torch.Tensor:
    """The already gathered `out` (rows j < n <- slot idx[j] of the newline grid over `flat` and `newline`; tail rows
    behind them) returned as the output of a differentiable gather with respect to `flat`, `newline` and `tail`."""
    spec = (idx, int(n), int(F), int(h), tuple(flat.shape), tuple(newline.shape),
            tuple(tail.shape) if tail is not None else None, bool(validate))
    return _GatherRowsGrid.apply(_Box(out.detach(), spec), flat, newline, tail)


class _GatherCols(torch.autograd.Function):
    @staticmethod
    def forward(ctx, box, x):
        ctx.idx, ctx.D = box.spec
        return box.outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return None, cols_grad(g, ctx.idx, ctx.D)


def attach_cols(out: torch.Tensor, x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """out = x[:, idx] (made by vc2_gather_cols) with its backward attached."""
    return _GatherCols.apply(_Box(out.detach(), (idx, int(x.shape[1]))), x)


class _Pool(torch.autograd.Function):
    """A pooled tensor made by the fused pool (fused.pool_stats), differentiated through the model's own pooling:
    the backward recomputes `pool(x)` and applies its Jacobian (exact for average and bilinear pooling, which are linear;
    max pooling routes a tie to the element the model's own pooling picks)."""

    @staticmethod
    def forward(ctx, box, x):
        ctx.pool = box.spec
        ctx.save_for_backward(x)
        return box.outs

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        with torch.enable_grad():
            xi = x.detach().requires_grad_()
            y = ctx.pool(xi)
        return None, torch.autograd.grad(y, xi, g.reshape(y.shape))[0]


def attach_pool(out: torch.Tensor, x: torch.Tensor, pool: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    return _Pool.apply(_Box(out.detach(), pool), x)

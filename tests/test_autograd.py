"""CPU: the gather backward entry points (vc2_rows_grad, vc2_cols_grad) are declared, exported and bound, refuse bad
arguments before touching a device, and the autograd gate only opens when a graph is recorded for an input that
requires grad."""
import ctypes
import os
import re

import pytest
import torch

from vidcom2_amd import _ffi
from vidcom2_amd import autograd as ag

from conftest import ROOT

NEW = ("vc2_rows_grad", "vc2_cols_grad")
ERR_ARG, ERR_UNSUPPORTED = -1, -3


def test_backward_symbols_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vc2.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_ffi.LIB_PATH)
    for n in NEW:
        assert re.search(rf"\bint {n}\s*\(", src), n
        assert hasattr(handle, n), n
        assert n in _ffi.EXPORTED_SYMBOLS
        assert getattr(_ffi.lib(), n).argtypes is not None


def _arr(kind, vals):
    return (kind * len(vals))(*vals)


def _rows(gd=(0x1000,), gdr=(8,), gs=(0x2000,), gsr=(8,), n_src=1, D=16, dt=1, idx=0x3000, n=4, row0=0, inv=0x4000,
          inv_len=8):
    vp = ctypes.c_void_p
    return _ffi.lib().vc2_rows_grad(_arr(vp, gd), _arr(ctypes.c_int64, gdr), _arr(vp, gs), _arr(ctypes.c_int64, gsr),
                                    n_src, D, dt, vp(idx), None, n, row0, vp(inv), inv_len, None, None)


@pytest.mark.parametrize("kw,rc", [
    (dict(n_src=0), ERR_ARG),
    (dict(n_src=9), ERR_ARG),
    (dict(dt=3), ERR_ARG),
    (dict(D=0), ERR_ARG),
    (dict(n=-1), ERR_ARG),
    (dict(row0=-1), ERR_ARG),
    (dict(gd=(0,)), ERR_ARG),                        # null gradient tensor
    (dict(gs=(0,)), ERR_ARG),
    (dict(gdr=(3,)), ERR_ARG),                       # fewer gradient rows than dst_row0 + n
    (dict(row0=5), ERR_ARG),
    (dict(inv=0), ERR_ARG),                          # an index list needs the inverse-map scratch ...
    (dict(inv_len=7), ERR_ARG),                      # ... of max(gsrc_rows) entries
    (dict(n=1 << 31, gdr=(1 << 32,)), ERR_UNSUPPORTED),
])
def test_rows_grad_refuses_bad_arguments_without_a_device(kw, rc):
    assert _rows(**kw) == rc
    assert _ffi.last_error()


def test_rows_grad_null_arrays():
    assert _ffi.lib().vc2_rows_grad(None, None, None, None, 1, 8, 1, None, None, 0, 0, None, 0, None, None) == ERR_ARG


@pytest.mark.parametrize("args,rc", [
    ((0, 4, 2, 4, 1, 0x1000, 0x2000), ERR_ARG),      # null g
    ((0x1000, 4, 2, 4, 1, 0, 0x2000), ERR_ARG),      # null idx
    ((0x1000, 4, 2, 4, 1, 0x3000, 0), ERR_ARG),      # null gx
    ((0x1000, 4, 5, 4, 1, 0x3000, 0x2000), ERR_ARG),  # C > D
    ((0x1000, 4, 0, 4, 1, 0x3000, 0x2000), ERR_ARG),
    ((0x1000, -1, 2, 4, 1, 0x3000, 0x2000), ERR_ARG),
    ((0x1000, 4, 2, 4, 7, 0x3000, 0x2000), ERR_ARG),  # dtype
    ((0x1000, 4, 2, 8193, 1, 0x3000, 0x2000), ERR_UNSUPPORTED),
])
def test_cols_grad_refuses_bad_arguments_without_a_device(args, rc):
    g, R, C, D, dt, idx, gx = args
    vp = ctypes.c_void_p
    assert _ffi.lib().vc2_cols_grad(vp(g), R, C, D, dt, vp(idx), vp(gx), None, None) == rc


def test_gate_opens_only_when_recording_for_a_float_input_that_requires_grad():
    x = torch.zeros(4, 3, requires_grad=True)
    y = torch.zeros(4, 3)
    assert ag.wants_grad(x) and ag.wants_grad(y, None, x)
    assert not ag.wants_grad(y) and not ag.wants_grad(None)
    assert not ag.wants_grad(torch.zeros(3, dtype=torch.int64))
    with torch.no_grad():
        assert not ag.wants_grad(x)
    with torch.inference_mode():
        assert not ag.wants_grad(x)

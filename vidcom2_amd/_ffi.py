"""ctypes binding of libvc2hip.so (the C ABI declared in include/vc2.h).

The library holds every hand-written gfx950 kernel of the hot path.  There is NO fallback:
if the shared object is missing or a tensor is not on a ROCm device the call raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VC2_LIB_PATH") or os.path.join(_PKG, "_lib", "libvc2hip.so")   # (override: A/B builds)

DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
MAP_LINEAR, MAP_GRID_VID, MAP_LOCAL = 0, 1, 2

_ERR_SHAPE, _ERR_UNSUPPORTED = -2, -3

_lib: Optional[ctypes.CDLL] = None

_vp, _i64, _i32, _dbl, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t

# name -> argtypes (restype int unless listed in _RESTYPES); mirrors include/vc2.h one to one
_SIGNATURES = {
    "vc2_workspace_bytes": [_i64, _i64, _i64, _i32, ctypes.POINTER(_sz)],
    "vc2_kept_capacity": [_i64, _i64, _dbl],
    "vc2_chan_var": [_vp, _i64, _i64, _i32, _vp, _sz, _vp, _vp, _vp],
    "vc2_chan_select": [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "vc2_gather_cols": [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp],
    "vc2_scores": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp],
    "vc2_compute_scales": [_vp, _i64, _dbl, _dbl, _i32, _vp, _sz, _vp, _vp],
    "vc2_select": [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp, _sz, _vp, _vp, _vp, _i64, _vp, _vp],
    "vc2_map_indices": [_vp, _vp, _vp, _i64, _i32, _i64, _vp, _vp],
    "vc2_gather_rows": [_vp, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp],
    "vc2_gather_rows_grid": [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp],
    "vc2_gather_rows_chunks": [_vp, _vp, _i32, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp],
    "vc2_gather_rows_grid_chunks": [_vp, _vp, _i32, _i64, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp],
    "vc2_compress": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                     _vp, _vp, _vp, _vp],
    "vc2_compress_ex": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                        _vp, _vp, _vp, _vp, _i64, _i32, _vp],
    "vc2_compress_ex2": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                         _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp],
    "vc2_compress_ex3": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                         _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "vc2_compress_ex4": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                         _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp],
    "vc2_compress_ex5": [_vp, _i64, _i64, _i64, _i32, _dbl, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _vp, _i64, _vp,
                         _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _vp, _vp],
    "vc2_wait_host_count": [_vp, _dbl],
    "vc2_pool_out_tokens": [_i64, _i64, _i32, _vp, _vp],
    "vc2_pool_stats": [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _sz, _vp, _vp],
    "vc2_pool_stats_blocks": [_vp, _i64, _i64, _i64, _i64, _i32, _i32, _i64, _i32, _vp, _sz, _vp, _vp, _vp, _vp],
    "vc2_gather_scatter": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp],
    "vc2_keep_positions": [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp],
    "vc2_keep_positions_batched": [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64,
                                   _vp, _i64, _vp, _vp, _vp, _vp, _vp],
    "vc2_repad_rows": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp],
    "vc2_rows_grad": [_vp, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp],
    "vc2_cols_grad": [_vp, _i64, _i64, _i64, _i32, _vp, _vp, _vp, _vp],
    "vc2_stat_block_frames": [],
    "vc2_chan_stats": [_vp, _i64, _i64, _i64, _i32, _i64, _i32, _vp, _sz, _vp, _vp],
    "vc2_chan_var_from_stats": [_vp, _i64, _i64, _i64, _i64, _i32, _vp, _vp, _vp],
    "vc2_scores_phase1": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _sz, _vp, _vp],
    "vc2_scores_phase2": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _sz, _vp, _vp,
                          _vp, _vp, _vp],
    "vc2_video_centre_blocks": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _sz,
                                _vp, _i32, _vp],
    "vc2_scores_phase2_blocks": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _sz, _vp,
                                 _vp, _vp, _vp, _vp, _i32, _i32, _vp],
    "vc2_video_centre_blocks_round": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _sz, _vp, _i32, _i32, _vp],
    "vc2_video_centre_flagged": [_i64, _i64, _i64, _i32, _i64, _vp, _sz, _vp, _vp],
    "vc2_video_centre_finish_round": [_i64, _i64, _i64, _i32, _i64, _vp, _i64, _vp, _sz, _vp, _i32, _i32, _i32, _vp],
    "vc2_video_centre_blocks_ragged": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i32,
                                       _i32, _vp, _sz, _vp, _i32, _vp],
    "vc2_video_centre_blocks_round_ragged": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _sz,
                                             _vp, _i32, _i32, _vp],
    "vc2_video_centre_finish_round_ragged": [_i64, _i64, _i64, _i32, _i64, _vp, _i64, _vp, _i32, _i32, _vp, _sz, _vp, _i32,
                                             _i32, _vp],
    "vc2_scores_phase2_blocks_ragged": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i32,
                                        _i32, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _i32, _vp],
    "vc2_select_sharded": [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _dbl, _i32, _vp, _sz, _vp, _vp, _i64, _vp, _vp,
                           _vp, _vp],
    "vc2_select_chunks_ws_bytes": [_i64, ctypes.POINTER(_sz)],
    "vc2_select_chunks": [_vp, _vp, _i64, _i64, _i64, _dbl, _i32, _vp, _sz, _vp, _sz, _i64, _vp, _vp, _i64, _vp, _vp, _vp,
                          _i32, _vp, _vp, _vp],
    "vc2_multi_scale_gaussian": [_vp, _i64, _i64, _i64, _i32, _vp, _i64, ctypes.POINTER(ctypes.c_double), _i32, _vp, _vp],
    "vc2_kat_exp": [_vp, _i64, _i32, _vp, _vp],
    "vc2_kat_round": [_vp, _i64, _i32, _vp, _vp],
    "vc2_set_mode": [_i32],
    "vc2_set_thread_mode": [_i32],
    "vc2_get_mode": [],
    "vc2_profile_enable": [_i32],
    "vc2_profile_collect": [_i32, _vp, _vp, _vp],
    "vc2_pass_counters": [_i64, _i64, _i64, _i32, _vp, _vp],
    "vc2_selftest_counters": [_vp, _i32],
    "vc2_selftest_force_guard": [_i32],
    "vc2_selftest_ord_pieces": [_i64, _i64, _i64, _i32, _vp, _i64],
    "vc2_selftest_margins": [_i64, _i32, _i32, _vp],
    "vc2_last_error": [],
    "vc2_version": [],
}
_RESTYPES = {"vc2_kept_capacity": _i64, "vc2_wait_host_count": _i64,  "vc2_last_error": ctypes.c_char_p, "vc2_version": ctypes.c_char_p}

# the frame-sharded entry points' `_o` forms: the plain signature and a trailing `const vc2_shard_opts*` (include/vc2.h)
for _name in ("vc2_chan_stats", "vc2_scores_phase1", "vc2_video_centre_blocks", "vc2_scores_phase2_blocks",
              "vc2_video_centre_blocks_round", "vc2_video_centre_finish_round", "vc2_video_centre_blocks_ragged",
              "vc2_video_centre_blocks_round_ragged", "vc2_video_centre_finish_round_ragged",
              "vc2_scores_phase2_blocks_ragged", "vc2_select_sharded", "vc2_select_chunks"):
    _SIGNATURES[_name + "_o"] = _SIGNATURES[_name] + [_vp]

# vc2_select_chunks_o and, behind the options: map_mode, grid_h, newline, tail, tail_rows
_SIGNATURES["vc2_select_chunks_x"] = _SIGNATURES["vc2_select_chunks_o"] + [_i32, _i64, _vp, _vp, _i64]

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def lib() -> ctypes.CDLL:
    """Load libvc2hip.so (built by __graft_entry__.build()); fail loudly if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"vidcom2_amd: HIP extension {LIB_PATH} is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU or PyTorch fallback for this path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, args in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.argtypes = args
            fn.restype = _RESTYPES.get(name, ctypes.c_int)
        _lib = handle
    return _lib


def last_error() -> str:
    return lib().vc2_last_error().decode("utf-8", "replace")


def check(rc: int, what: str) -> None:
    if rc == 0:
        return
    msg = last_error()
    if rc == _ERR_SHAPE:
        raise RuntimeError(f"{what}: {msg}")
    if rc == _ERR_UNSUPPORTED:
        raise NotImplementedError(f"{what}: {msg}")
    raise RuntimeError(f"{what} failed (code {rc}): {msg}")


def require_device(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(
            f"vidcom2_amd: {what} lives on {t.device}; this package only runs its HIP kernels on a ROCm "
            "device (torch device type 'cuda'). There is no CPU fallback -- move the tensor to the GPU.")
    if t.dtype not in DTYPE_CODE and t.dtype != torch.int64 and t.dtype != torch.uint8 and t.dtype != torch.float64:
        raise TypeError(f"{what}: unsupported dtype {t.dtype} (fp32 / bf16 / fp16 only)")


def on_device(device):
    """Context: make `device` the current HIP device for the duration of a library call.  The C ABI launches on the
    stream it is given but keys per-device state (LDS opt-in, events) on the CURRENT device, and a tensor may live on
    a GPU that is not current (HF device_map='auto' puts the vision tower's output anywhere)."""
    return _OnDevice(device)


class _OnDevice:
    """torch.cuda.device(device), but free when `device` is current already (the usual case: three nested guards on
    the one-shot path cost ~12 us of hipGetDevice / hipSetDevice pairs)."""
    __slots__ = ("_idx", "_ctx")

    def __init__(self, device):
        d = torch.device(device) if not isinstance(device, int) else None
        self._idx = device if d is None else d.index
        self._ctx = None

    def __enter__(self):
        if self._idx is not None and torch.cuda.current_device() != self._idx:
            self._ctx = torch.cuda.device(self._idx)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
            self._ctx = None
        return False


def ptr(t: Optional[torch.Tensor]) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def stream_ptr(device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def workspace_bytes(F: int, N: int, D: int, dtype) -> int:
    out = _sz(0)
    check(lib().vc2_workspace_bytes(F, N, D, DTYPE_CODE[dtype], ctypes.byref(out)), "vc2_workspace_bytes")
    return int(out.value)


def workspace(F: int, N: int, D: int, dtype, device) -> torch.Tensor:
    return torch.empty(workspace_bytes(F, N, D, dtype), dtype=torch.uint8, device=device)


def profile_enable(on: bool) -> None:
    check(lib().vc2_profile_enable(int(bool(on))), "vc2_profile_enable")


def profile_collect() -> dict:
    """{kernel name: (total_ms, launches)} accumulated since profile_enable(True)."""
    n = 32
    names = (ctypes.c_char_p * n)()
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_int64 * n)()
    got = lib().vc2_profile_collect(n, names, ms, cnt)
    return {names[i].decode(): (float(ms[i]), int(cnt[i])) for i in range(got) if cnt[i]}


# 'torch' = the library default (C mode 4): bit-exact to the CPU reference; the frame-mean replay margin has a term relative
# to sum |x^| so that it grows under cancellation.  'torch_proven' (mode 3): a PROVEN error bound decides which centre
# means are replayed -- same results (the parity suite asserts that on every fixture) at ~45 % more time per pass (round 5:
# 256 against 178 us at the target shape).
# 'torch_fast' (mode 1, the default of rounds 1-3): the 16-ulp empirical margin alone, ~1 % faster, NOT bit-exact on
# adversarial cancellation inputs -- opt-in, no parity claim.  ('torch_robust': the name mode 4 had while it was opt-in.)
MODE_CODE = {"exact": 0, "torch": 4, "torch_fast": 1, "torch_proven": 3, "torch_robust": 4}


def set_mode(mode: str) -> None:
    """'torch' (default): bit-exact to the CPU reference in half precision (replays torch's fp32 accumulation
    order where it decides a rounding; for fp16 token norms within an empirical margin); 'exact': every
    reduction correctly rounded; 'torch_proven': proven margins for all centre means and fp16 norms (~45 % slower); 'torch_fast': empirical margins only (opt-in, no parity claim under cancellation).
    get_mode() answers 'torch' for all torch modes."""
    check(lib().vc2_set_mode(MODE_CODE[mode]), "vc2_set_mode")


def set_thread_mode(mode: Optional[str]) -> None:
    """Override the process-wide mode for the calling thread only; None: follow the process-wide setting again."""
    check(lib().vc2_set_thread_mode(-1 if mode is None else MODE_CODE[mode]), "vc2_set_thread_mode")


def get_mode() -> str:
    return "torch" if lib().vc2_get_mode() else "exact"

"""MI355X-native mirror of the reference plugin API ``token_compressor/vidcom2/vidcom2.py``.

Same function names, argument meaning, return types and error behaviour as the reference
(file:line cited per function); the tensor work is done by the gfx950 HIP kernels in
``csrc/vc2_kernels.hip`` through the C ABI of ``include/vc2.h``.  PyTorch is used only to
allocate device memory and to supply the current HIP stream.

Numerics: like the reference, every op runs "in the input dtype" -- see DESIGN.md
"Numerics contract".  Inputs are never modified; every return value is a fresh tensor on the
input's device.  Tensors must live on a ROCm device: there is no CPU fallback.
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import math
import os
import threading
import time
import warnings
from dataclasses import dataclass
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import torch

from . import _ffi
from . import autograd as _ag
from ._ffi import DTYPE_CODE, MAP_GRID_VID, MAP_LINEAR, MAP_LOCAL, check, lib, on_device, ptr, require_device, stream_ptr

# vidcom2.py:7-13 -- 'mapper' selects the index mapping, 'tpf' the default tokens per frame
# (None = provided per call through frame_token_len).
MODEL_SPECS: Dict[str, Dict[str, Any]] = {
    "llava_ov": {"tpf": 196, "mapper": "linear"},
    "llava_vid": {"tpf": 169, "mapper": "grid_vid", "grid": 13},
    "qwen2_vl": {"tpf": None, "mapper": "linear"},
    "qwen2_5_vl": {"tpf": None, "mapper": "linear"},
    "qwen3_vl": {"tpf": None, "mapper": "linear"},
}
_DYNAMIC_TPF = {"qwen2_vl", "qwen2_5_vl", "qwen3_vl"}
_ALPHAS = [2 ** k for k in range(-3, 2)]          # vidcom2.py:54


_MAX_ALPHAS = 16                                   # include/vc2.h: vc2_pass_params.alphas
_MAX_CHANNELS = 4096                               # scored channels the sweeps cover (64 compact positions per lane)


class _CPassParams(ctypes.Structure):
    """include/vc2.h: vc2_pass_params."""
    _fields_ = [("channels", ctypes.c_int64), ("temp", ctypes.c_double), ("n_alphas", ctypes.c_int32),
                ("alphas", ctypes.c_double * _MAX_ALPHAS)]


class PassParams:
    """The method's three hyper-parameters besides the retention ratio, for the one-launch pass (`compress`,
    `compress_batch`, `CompressPlan`): the share of low-variance channels that are scored (`select_low_var_channels`'
    ratio, vidcom2.py:38), the temperature of the budget softmax (`compute_scales`' temp, vidcom2.py:64) and the
    Gaussian scales (vidcom2.py:54) in the order Python's `sum()` adds their terms.  Immutable and hashable; validated
    here, on the host.  An instance equal to the reference's defaults is the default pass (`is_default`): it shares
    kernels, bits and cached plans with a call without params."""
    __slots__ = ("channel_ratio", "temp", "alphas")

    def __init__(self, channel_ratio: float = 0.5, temp: float = 0.01, alphas=(0.125, 0.25, 0.5, 1.0, 2.0)):
        try:
            ratio, t, al = float(channel_ratio), float(temp), tuple(float(a) for a in alphas)
        except (TypeError, ValueError) as e:
            raise ValueError(f"PassParams: {e}") from None
        if not (0.0 < ratio <= 1.0):                     # (NaN fails the comparison too)
            raise ValueError(f"PassParams: channel_ratio {channel_ratio!r} outside (0, 1]")
        if not (t > 0.0 and math.isfinite(t)):
            raise ValueError(f"PassParams: temp {temp!r} must be finite and > 0")
        if not al:
            raise ValueError("PassParams: alphas is empty")
        if any(not (a > 0.0 and math.isfinite(a)) for a in al):
            raise ValueError(f"PassParams: every alpha must be finite and > 0, got {list(alphas)!r}")
        if len(al) > _MAX_ALPHAS:
            raise NotImplementedError(f"PassParams: {len(al)} Gaussian scales; the pass takes at most {_MAX_ALPHAS}")
        object.__setattr__(self, "channel_ratio", ratio)
        object.__setattr__(self, "temp", t)
        object.__setattr__(self, "alphas", al)

    def __setattr__(self, name, value):
        raise AttributeError("PassParams is immutable")

    def __delattr__(self, name):
        raise AttributeError("PassParams is immutable")

    def _key(self):
        return (self.channel_ratio, self.temp, self.alphas)

    def __eq__(self, other):
        return isinstance(other, PassParams) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return f"PassParams(channel_ratio={self.channel_ratio!r}, temp={self.temp!r}, alphas={self.alphas!r})"

    def __reduce__(self):
        return (PassParams, self._key())

    def channels(self, D: int) -> int:
        """int(D * ratio): the number of channels the reference scores (vidcom2.py:41)."""
        return int(int(D) * self.channel_ratio)

    @property
    def is_default(self) -> bool:
        return self._key() == _DEFAULT_PARAMS_KEY


_DEFAULT_PARAMS_KEY = (0.5, 0.01, tuple(float(a) for a in _ALPHAS))


def _norm_params(params: Optional["PassParams"]) -> Optional["PassParams"]:
    """None for the reference's defaults ("no params": the plain call, its kernels and its cached plans)."""
    if params is None:
        return None
    if not isinstance(params, PassParams):
        raise TypeError(f"params must be a PassParams, got {type(params).__name__}")
    return None if params.is_default else params


def _c_params(params: Optional["PassParams"], D: int) -> Optional[_CPassParams]:
    """vc2_pass_params of a normalised PassParams for rows of D channels; the C ABI's own limits, raised before anything
    is allocated."""
    if params is None:
        return None
    C = params.channels(D)
    if C < 1:
        raise ValueError(f"channel_ratio {params.channel_ratio} selects no channel of {D} (int({D} * ratio) == 0)")
    if C > _MAX_CHANNELS:
        raise NotImplementedError(f"channel_ratio {params.channel_ratio} selects {C} of {D} channels; the pass scores at "
                                  f"most {_MAX_CHANNELS}")
    return _CPassParams(C, params.temp, len(params.alphas), (ctypes.c_double * _MAX_ALPHAS)(*params.alphas))


def _norm_score_dtype(score_dtype, dtype) -> Optional[torch.dtype]:
    """None for "score in the input's dtype" (score_dtype None or equal to it: the plain call, its kernels and its cached
    plans); torch.float32 over a bf16 / fp16 tensor: the fp32-scored pass (vc2_compress_ex4)."""
    if score_dtype is None or score_dtype == dtype:
        return None
    if score_dtype == torch.float32 and dtype in (torch.bfloat16, torch.float16):
        return torch.float32
    raise ValueError(f"score_dtype must be None, the input's dtype ({dtype}) or torch.float32 over a bfloat16 / float16 "
                     f"tensor, got {score_dtype!r}")


def _first_tensor(a):
    if isinstance(a, torch.Tensor):
        return a
    if isinstance(a, (list, tuple)) and a and isinstance(a[0], torch.Tensor):
        return a[0]
    return None


def _guarded(fn):
    """Run `fn` with the device of its first tensor argument current (see _ffi.on_device)."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        t = next((x for x in map(_first_tensor, args) if x is not None), None)
        if t is None or t.device.type != "cuda":
            return fn(*args, **kwargs)
        with on_device(t.device):
            return fn(*args, **kwargs)
    return wrapper


def _as_int(v) -> int:
    if isinstance(v, torch.Tensor):
        return int(v.reshape(-1)[0].item()) if v.numel() == 1 else int(v)
    return int(v)


def _prep(x: torch.Tensor, what: str) -> torch.Tensor:
    require_device(x, what)
    if x.dtype not in DTYPE_CODE:
        raise TypeError(f"{what}: unsupported dtype {x.dtype} (fp32 / bf16 / fp16 only)")
    if not x.is_contiguous():
        return x.contiguous()
    # include/vc2.h: base pointers are 16-byte aligned (the sweeps load whole 16-byte vectors).  torch's allocations are;
    # a view into one (a row slice of an odd-width tensor, a storage offset) need not be: it is copied
    return x if x.data_ptr() % 16 == 0 else x.clone()


def _prep_newline(newline, D: int, dtype, device) -> torch.Tensor:
    """The grid mapping's newline vector (the model's `image_newline`) as the [D] tensor the gather launch reads: [D] or
    [1, D], the input's dtype, on its device.  A non-contiguous one is copied; a misaligned one (a view at an odd element
    offset) is NOT: the gather takes its scalar copy path for those rows."""
    device = torch.device(device)
    if not isinstance(newline, torch.Tensor) or tuple(newline.shape) not in ((D,), (1, D)) or newline.dtype != dtype \
            or newline.device.type != device.type or (device.index is not None and newline.device.index != device.index):
        got = f"{tuple(newline.shape)} {newline.dtype} on {newline.device}" if isinstance(newline, torch.Tensor) \
            else type(newline).__name__
        raise RuntimeError(f"newline must be a [{D}] or [1, {D}] {dtype} tensor on {device}, got {got}")
    newline = newline.detach().reshape(D)
    return newline if newline.is_contiguous() else newline.contiguous()


@dataclass
class CompressionResult:
    """Everything one pass produces (device tensors; ``K`` / ``ks`` are synced to host lazily)."""
    rows: Optional[torch.Tensor]        # [K, D] gathered rows (None when no gather was requested)
    global_idx: torch.Tensor            # int64 [K] mapped global indices
    ks: torch.Tensor                    # int64 [F] per-frame budgets
    K: int
    v_score: Optional[torch.Tensor] = None   # T [F, N]
    f_score: Optional[torch.Tensor] = None   # T [F, N]


def cascade_level_power(n: int) -> int:
    """torch's SumKernel.cpp level_power for a reduction over n elements: max(4, ceil_log2(n) // 4) -- 4 up to 2^19
    elements, 5 up to 2^23, 6 up to 2^27 (the block size 2^lp of the centre-mean replays, csrc cascade_lp)."""
    return max(4, (max(int(n), 1) - 1).bit_length() // 4)


def cascade_modelled(n: int) -> bool:
    """Is torch's summation order for a centre mean over n tokens replayed by the kernels (csrc cascade_modelled)?"""
    lp = cascade_level_power(n)
    return lp <= 6 and (((int(n) >> lp) + (1 << lp) - 1) >> lp) <= 8192


class OutputSet(NamedTuple):
    """The output tensors one pass writes (a plan's own, a fresh set per one-shot call, or one clip's slice of
    compress_batch's batch-wide buffers): kept indices, budgets, kept rows (+ tail rows), scores, (K, status) words."""
    idx: torch.Tensor                   # int64 [cap]
    ks: torch.Tensor                    # int64 [F]
    rows: Optional[torch.Tensor]        # T [cap + tail_rows, D] (None: no gather)
    v: Optional[torch.Tensor]           # T [F, N] (None: no scores)
    f: Optional[torch.Tensor]
    kout: torch.Tensor                  # int64 [2]: (K, status), both written by every pass

    def result(self, K, status) -> CompressionResult:
        """The pass's result once its (K, status) words are on the host: raises on a nonzero status."""
        K, cap = int(K), self.idx.shape[-1]
        if status:
            _raise_status(int(status), cap, K)
        rows = None if self.rows is None else self.rows[:K + self.rows.shape[0] - cap]     # (+ the tail rows)
        return CompressionResult(rows, self.idx[:K], self.ks, K, self.v, self.f)


class _LateStatus(NamedTuple):
    """A pass that finish() returned on the early words of its pinned mirror block: its final status word is still to be
    read (CompressPlan._settle)."""
    block: "_KHost"
    cap: int
    K: int
    stream: "torch.cuda.Stream"         # the stream the pass was enqueued on


class CompressPlan:
    """Pre-allocated buffers for repeated passes over one (F, N, D, dtype) shape.

    ``enqueue`` launches the whole pass (8 kernels, no host round trip) on the current stream;
    ``finish`` performs the path's single device->host sync (the reference's ``.tolist()``,
    vidcom2.py:72) and slices the outputs to the K kept tokens.
    """

    def __init__(self, F: int, N: int, D: int, dtype, device, base_scale: float = 0.25,
                 mapper: str = "linear", grid_h: int = 0, want_scores: bool = False, gather: bool = True,
                 tail_rows: int = 0, ws: Optional[torch.Tensor] = None, score_dtype: Optional[torch.dtype] = None,
                 params: Optional[PassParams] = None):
        if mapper not in ("linear", "grid_vid"):
            raise ValueError(f"unknown mapper {mapper!r}")
        self.F, self.N, self.D, self.dtype, self.device = int(F), int(N), int(D), dtype, torch.device(device)
        # the dtype the pass rounds in: the input's, or fp32 over 16-bit rows (the reference on x.float(), no fp32 copy)
        self.score_dtype = _norm_score_dtype(score_dtype, dtype)
        self.arith_dtype = dtype if self.score_dtype is None else self.score_dtype
        self.params = _norm_params(params)               # None: the reference's hyper-parameters
        self._cparams = _c_params(self.params, self.D)
        self.base_scale = float(base_scale)
        self.map_mode = MAP_LINEAR if mapper == "linear" else MAP_GRID_VID
        self.grid_h = int(grid_h)
        L = lib()
        cap = int(L.vc2_kept_capacity(self.F, self.N, self.base_scale))
        if self.map_mode == MAP_GRID_VID:
            cap += self.F * self.grid_h
        self.cap = cap
        if self.arith_dtype != torch.float32 and _ffi.get_mode() == "torch" and not cascade_modelled(self.F * self.N):
            # beyond this size the centre-mean replays do not model torch's outer-sum cascade (SumKernel.cpp level_power
            # 4 / 5 / 6 are modelled, i.e. up to 2^25 tokens per video): say so instead of silently keeping the exactly
            # rounded means
            warnings.warn(f"vidcom2_amd: {self.F} x {self.N} tokens exceed the modelled range of torch's centre-mean "
                          "accumulation order (2^25 tokens per video); boundary-near centre values "
                          "keep their exactly rounded mean and may differ from the CPU reference by one ulp",
                          RuntimeWarning, stacklevel=3)
        self.ws = ws if ws is not None else _ffi.workspace(self.F, self.N, self.D, dtype, self.device)
        # tail_rows: extra rows (LLaVA's newline embedding) the gather launch appends behind the kept ones
        self.tail_rows = int(tail_rows) if gather else 0
        self._gather, self._want_scores = bool(gather), bool(want_scores)
        self.out = self._alloc_outputs()                 # the plan's own output set (enqueue without `out`, finish)
        self._spare = None
        # (K, status) mirrored by the selection launch into pinned host memory (vc2_compress_ex2): finish(early=True) gets
        # the count from there -- ~15 us before the pass ends, no device-to-host copy -- and returns while the gather runs
        self._khost = None
        self._armed = None                               # the stream of a mirrored pass that finish() has not seen yet
        self._late = None                                # _LateStatus: read and cleared by _settle alone
        self._settle_lock = threading.Lock()

    # the plan's own outputs, read-only: a caller that wants the pass written elsewhere passes `enqueue(..., out=)`
    idx = property(lambda self: self.out.idx)
    ks = property(lambda self: self.out.ks)
    rows = property(lambda self: self.out.rows)
    v = property(lambda self: self.out.v)
    f = property(lambda self: self.out.f)
    kout = property(lambda self: self.out.kout)

    def _alloc_outputs(self, n: Optional[int] = None) -> OutputSet:
        """A fresh output set; with n: n sets in ONE allocation per output kind ([n, ...] tensors: compress_batch)."""
        dt, dev, lead = self.dtype, self.device, () if n is None else (n,)     # (sizes as arguments: ~1 us less each)
        sdt = self.arith_dtype                                                 # (scores: the dtype the pass rounds in)
        return OutputSet(torch.empty(*lead, self.cap, dtype=torch.int64, device=dev),
                         torch.empty(*lead, self.F, dtype=torch.int64, device=dev),
                         torch.empty(*lead, self.cap + self.tail_rows, self.D, dtype=dt, device=dev) if self._gather else None,
                         torch.empty(*lead, self.F, self.N, dtype=sdt, device=dev) if self._want_scores else None,
                         torch.empty(*lead, self.F, self.N, dtype=sdt, device=dev) if self._want_scores else None,
                         torch.empty(*lead, 2, dtype=torch.int64, device=dev))

    def new_outputs(self) -> None:
        """A fresh own output set (kept rows, indices, budgets, scores) for the next pass.  A plan that is re-used for
        independent calls (the one-shot API's plan cache) takes one before every enqueue, so that a result handed out
        earlier is never overwritten -- the reference returns fresh tensors as well; workspace and status words stay.
        (`prepare_spare` may have made the set already, while the previous pass was running.)"""
        spare, self._spare = self._spare, None
        self.out = spare if spare is not None else self._alloc_outputs()

    def output_bytes(self) -> int:
        """Bytes of ONE output set (kept rows, indices, budgets, scores, status words)."""
        es = torch.empty(0, dtype=self.dtype).element_size()
        n = self.cap * 8 + self.F * 8 + 16
        if self._gather:
            n += (self.cap + self.tail_rows) * self.D * es
        if self._want_scores:
            n += 2 * self.F * self.N * torch.empty(0, dtype=self.arith_dtype).element_size()
        return n

    def cached_bytes(self) -> int:
        """What a cached plan keeps alive: workspace, the last output set, the spare one."""
        return int(self.ws.numel()) + self.output_bytes() * (2 if self._spare is not None else 1)

    def prepare_spare(self) -> None:
        """Allocate the NEXT call's output tensors now -- called by the one-shot API between enqueue and finish, i.e.
        while the GPU is busy with this pass -- so that the next call launches its first kernel ~25 us earlier (five
        allocations).  Still fresh tensors per call: nothing a caller holds is ever overwritten."""
        if self._spare is None:
            self._spare = self._alloc_outputs()

    def enqueue(self, flat: torch.Tensor, gather_src: Optional[torch.Tensor] = None,
                tail: Optional[torch.Tensor] = None, have_stats: bool = False, mirror: bool = False,
                stream: Optional["torch.cuda.Stream"] = None, out: Optional[OutputSet] = None,
                newline: Optional[torch.Tensor] = None) -> None:
        """have_stats: `self.ws` already holds flat's sweep-1 partials (fused.pool_stats wrote them on this
        stream), so the pass starts at the variance reduction.  mirror: the count is also written to pinned host
        memory (finish(early=True)).  out: the output set to write (one this plan's `_alloc_outputs` could have made;
        the caller reads it) instead of the plan's own.  newline (grid_vid plans, instead of gather_src): the model's
        [D] newline embedding -- the gather reads the kept rows from `flat` and the newline rows from the vector, the
        [F*h*(h+1), D] stream is never built (vidcom2.py:93-96, :105-115).  The pointer belongs to this call alone:
        nothing of it stays in the plan."""
        if newline is not None:
            if self.map_mode != MAP_GRID_VID:
                raise ValueError("newline is the grid_vid mapper's newline vector; this plan maps linearly")
            if gather_src is not None:
                raise ValueError("give either gather_src (img_feat) or newline, not both")
            newline = _prep_newline(newline, self.D, self.dtype, self.device)
        src = flat if gather_src is None else gather_src
        o = self.out if out is None else out
        if have_stats:
            tag = getattr(self.ws, "_vc2_stats_for", None)
            if tag is not None and tag != (self.F, self.N, self.D, self.dtype, flat.data_ptr()):
                raise RuntimeError(f"have_stats: the workspace holds the statistics of a {tag[:4]} tensor, not of this "
                                   f"({self.F}, {self.N}, {self.D}, {self.dtype}) one")
        if self.tail_rows:
            if tail is None or tail.shape != (self.tail_rows, self.D) or tail.dtype != self.dtype \
                    or tail.device != self.device:
                raise RuntimeError(f"tail must be [{self.tail_rows}, {self.D}] {self.dtype} on {self.device}")
            tail = tail.contiguous()
        khost = None
        self._settle()                                   # (a previous pass that returned on its early status words: ANY next
        #                                                   enqueue of the plan reads its final word first, mirrored or not)
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        if mirror:
            if self._khost is None:
                self._khost = _khost_get()               # (pinned words from the process-wide pool: never freed)
            kh = self._khost
            kh.word.value = -1                           # (host write: the previous pass of this plan was settled)
            kh.final.value = 0
            kh.in_flight = True
            khost = kh.addr
        self._armed = st if mirror else None
        with on_device(self.device):
            rc = lib().vc2_compress_ex5(ptr(flat), self.F, self.N, self.D, DTYPE_CODE[self.dtype], self.base_scale,
                                        self.map_mode, self.grid_h, ptr(src if o.rows is not None else None),
                                        src.shape[0], ptr(self.ws), self.ws.numel(), ptr(o.rows), ptr(o.idx),
                                        self.cap, ptr(o.ks), ptr(o.kout), ptr(o.v), ptr(o.f),
                                        ptr(tail if self.tail_rows else None), self.tail_rows,
                                        1 if have_stats else 0, khost,
                                        None if self._cparams is None else ctypes.addressof(self._cparams),
                                        DTYPE_CODE[self.arith_dtype], ptr(newline), ctypes.c_void_p(st.cuda_stream))
        if rc != 0 and mirror:                           # (nothing was launched: the mirror block is not in flight)
            self._khost.in_flight = False
            self._armed = None
        check(rc, "vc2_compress")

    def settle_quietly(self) -> None:
        """The last word on a pass that returned on its early status words, for the places that must not raise -- the
        plan is dropped (`__del__`), evicted from or cleared out of the plan cache, or the process ends: a late
        selection-guard hit is REPORTED there (RuntimeWarning; a "cannot happen" bit -- the caller's result is already
        in its hands), where `_settle` raises it in front of the plan's next pass."""
        try:
            self._settle()
        except RuntimeError as e:
            warnings.warn(f"vidcom2_amd: {e}", RuntimeWarning, stacklevel=2)
        except Exception:                                # (interpreter shutdown: torch half gone)
            pass

    def __del__(self):
        self.settle_quietly()
        kh = getattr(self, "_khost", None)
        if kh is not None:
            try:
                _khost_put(kh)
            except Exception:                            # (interpreter shutdown)
                pass

    def finish(self) -> CompressionResult:
        # (spinning on an event behind a copy to pinned memory instead of this blocking copy: measured, no gain -- torch's
        #  blocking copy already spins)
        out, st, self._armed = self.out, self._armed, None
        if st is not None:
            # the count from the pinned mirror: the caller goes on (slicing, the next launches) while the gather launch is
            # still running -- everything it does with these tensors is ordered by the stream, like the reference's
            # tensors after its `.tolist()`.  Falls back to the blocking copy after 50 ms.
            kh = self._khost
            K = int(lib().vc2_wait_host_count(kh.addr, 0.05))
            if K >= 0:
                # the launch's FINAL status word arrives when its last selection ends (~10 us after K): taken if it is
                # there already, else this pass is settled before the plan's next one starts (_settle) -- a late
                # selection-guard hit is raised there, never lost
                early, final = _mirror_words(kh)
                if final is None and not early:
                    self._late = _LateStatus(kh, self.cap, K, st)
                    return out.result(K, 0)
                if final is None:                        # (a fault in the early words, raised here once: the block is
                    st.synchronize()                     #  quiet before the plan's next pass re-arms it)
                    final = _mirror_words(kh)[1]
                return out.result(K, early if final is None else final)
        K, status = out.kout.tolist()                    # the single host sync of the path
        return out.result(K, status)

    def _settle(self) -> None:
        """A pass that returned on the early status words of the host mirror: read its final status word now and raise
        what it reports.  The only reader of the pending record: owner and a thread that evicts the plan claim it under
        the lock, so that exactly one of them reports it, and the block is read before the owner can re-arm it.  A word
        that has not arrived yet is waited for on the stream the pass was enqueued on."""
        with self._settle_lock:
            p, self._late = self._late, None
            if p is None:
                return
            status = _mirror_words(p.block)[1]
            if status is None:
                p.stream.synchronize()
                status = _mirror_words(p.block)[1]
        try:
            if status is None:
                raise RuntimeError("vidcom2_amd: no final status word after its stream was synchronised -- please report")
            if status:
                _raise_status(status, p.cap, p.K)
        except RuntimeError as e:
            raise RuntimeError(f"the PREVIOUS pass of this plan (its result was already returned): {e}") from None


# ---- plan cache of the one-shot API --------------------------------------------------------------------------
# `compress()` / `vidcom2_compression()` / the model hooks run one pass per call; building a CompressPlan (a ~30 MB
# workspace, status words) costs more than a quarter of the pass.  Plans are therefore kept per (shape, dtype, device,
# options, HIP stream, thread): work enqueued on ONE stream is ordered, so re-using a plan's workspace there is safe;
# another stream or thread gets its own plan.  Outputs are NOT cached (`fresh_outputs`: CompressPlan.new_outputs).
_PLAN_CACHE: "collections.OrderedDict" = collections.OrderedDict()
_PLAN_CACHE_MAX = int(os.environ.get("VC2_PLAN_CACHE", "8"))       # 0 disables the cache
_PLAN_CACHE_BYTES = int(os.environ.get("VC2_PLAN_CACHE_MB", "1024")) << 20   # workspaces + output sets kept alive by the cache
_SPARE_MAX_BYTES = int(os.environ.get("VC2_SPARE_MAX_MB", "256")) << 20      # no spare output set beyond this size
_PLAN_LOCK = threading.Lock()
_EARLY_COUNT = os.environ.get("VC2_EARLY_COUNT", "1") != "0"        # one-shot calls take K from a pinned host mirror (vc2_compress_ex2)
_PREALLOC = os.environ.get("VC2_PREALLOC", "1") != "0"             # next call's outputs allocated while this pass runs


def _cached_plan(F, N, D, dtype, device, base_scale, mapper, grid_h, want_scores, gather, tail_rows,
                 fresh_outputs: bool = False, params: Optional[PassParams] = None,
                 score_dtype: Optional[torch.dtype] = None) -> "CompressPlan":
    device = torch.device(device)
    params = _norm_params(params)
    score_dtype = _norm_score_dtype(score_dtype, dtype)      # (None / the input's dtype: the plain call's key and plan)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    key = (F, N, D, dtype, device, float(base_scale), mapper, int(grid_h), bool(want_scores), bool(gather),
           int(tail_rows), torch.cuda.current_stream(device).cuda_stream, threading.get_ident(), _ffi.get_mode(), params, score_dtype)
    # (the key holds the thread id, so a plan is only ever USED by one thread; the dictionary itself is shared: another
    #  thread's eviction between get and move_to_end raised KeyError before the lock)
    with _PLAN_LOCK:
        plan = _PLAN_CACHE.get(key) if _PLAN_CACHE_MAX > 0 else None
        if plan is not None:
            _PLAN_CACHE.move_to_end(key)
    if plan is None:
        plan = CompressPlan(F, N, D, dtype, device, base_scale, mapper, grid_h, want_scores, gather, tail_rows,
                            params=params, score_dtype=score_dtype)
        if _PLAN_CACHE_MAX > 0:
            with _PLAN_LOCK:
                _PLAN_CACHE[key] = plan
                # bounded by entries AND by bytes (a long clip's workspace is hundreds of MB): oldest first
                # (a cached plan keeps its workspace AND its last output set, plus a spare one: all counted)
                evicted = []
                while len(_PLAN_CACHE) > _PLAN_CACHE_MAX or \
                        (len(_PLAN_CACHE) > 1 and sum(p.cached_bytes() for p in _PLAN_CACHE.values()) > _PLAN_CACHE_BYTES):
                    evicted.append(_PLAN_CACHE.popitem(last=False)[1])
            for old in evicted:               # (outside the lock: may wait for another thread's stream)
                old.settle_quietly()          # a pass that returned on its early status words gets its last word here
    elif fresh_outputs:
        plan.new_outputs()
    return plan


def clear_plan_cache() -> None:
    with _PLAN_LOCK:
        plans = list(_PLAN_CACHE.values())
        _PLAN_CACHE.clear()
    for p in plans:
        p.settle_quietly()


atexit.register(clear_plan_cache)            # (the last call of the process: its final status word is read, not lost)


class _KHost:
    """Four pinned int64 words for vc2_compress_ex2's host mirror (K, early status, final status | 2^62, spare).  Pooled
    and never freed: the selection launch writes the final word ~10 us after the count, possibly after the plan that
    enqueued the pass is gone -- a block handed back to the allocator could be somebody else's memory by then."""
    __slots__ = ("t", "addr", "word", "early", "final", "in_flight")

    def __init__(self):
        self.t = torch.zeros(4, dtype=torch.int64).pin_memory()
        self.addr = ctypes.c_void_p(self.t.data_ptr())
        self.word, self.early, self.final = (ctypes.c_int64.from_address(self.t.data_ptr() + 8 * i) for i in range(3))
        self.in_flight = False


def _mirror_words(b: _KHost) -> Tuple[int, Optional[int]]:
    """(early status, final status -- None while the launch has not written it) of a mirror block: every read of a
    pass's status from these words goes through here (the tests replace it to force the late path)."""
    fin = b.final.value
    return b.early.value, (fin & ~_STATUS_FINAL if fin & _STATUS_FINAL else None)


_KHOST_LOCK = threading.RLock()       # (re-entrant: a garbage collection inside the locked region may finalise a plan -> _khost_put)
_KHOST_FREE: list = []
_KHOST_QUARANTINE: list = []         # returned while their pass may still write the final word


def _khost_get() -> _KHost:
    with _KHOST_LOCK:
        still = []
        for b in _KHOST_QUARANTINE:
            (_KHOST_FREE if b.final.value & _STATUS_FINAL else still).append(b)
        _KHOST_QUARANTINE[:] = still
        b = _KHOST_FREE.pop() if _KHOST_FREE else None
    if b is None:
        b = _KHost()
    b.in_flight = False
    return b


def _khost_put(b: _KHost) -> None:
    with _KHOST_LOCK:
        (_KHOST_QUARANTINE if b.in_flight and not (b.final.value & _STATUS_FINAL) else _KHOST_FREE).append(b)


_STATUS_FINAL = 1 << 62          # K_host[2] of vc2_compress_ex2: "this is the launch's final status word"


_BUDGET_CAN_EXCEED: Dict[Tuple[int, Any], bool] = {}


def _check_budgets(ks: torch.Tensor, N: int, dtype) -> None:
    """The reference's budgets are round(RN_T(scale * N)) (vidcom2.py:72): with scale = 1.0 and an N that is not a T
    value (bf16: N > 256 with more than 8 significant bits, e.g. 8188 -> 8192; fp16: N > 2048 with more than 11) a budget
    exceeds the frame and torch.topk raises.  The kernels report the raw budget in `ks` and select min(k, N) tokens; the
    device read that turns this into the reference's error is only made for such N (no budget can exceed any other N,
    as scale <= 1)."""
    key = (int(N), dtype)
    can = _BUDGET_CAN_EXCEED.get(key)
    if can is None:
        can = _BUDGET_CAN_EXCEED[key] = float(torch.tensor(float(N)).to(dtype)) != float(N)
    if can and int(ks.max()) > N:
        raise RuntimeError("selected index k out of range")


def _raise_status(status: int, cap: int, K: int) -> None:
    """K_out[1] of a pass (include/vc2.h): every bit is a 'cannot happen' condition the kernels check for instead of
    returning a silently wrong kept set."""
    why = []
    if status & 1:
        why.append(f"kept-token capacity {cap} exceeded (K={K}): vc2_kept_capacity bound violated")
    if status & 2:
        why.append("a bounded wait between workgroups of one launch expired")
    if status & 4:
        why.append("a loop bound of the selection replay expired (vc2_selftest_counters has the details)")
    if status & ~7:
        why.append(f"unknown status bits {status:#x}")
    raise RuntimeError("vidcom2_amd: " + "; ".join(why) + " -- please report")


@_guarded
def compress(flattened_feat: torch.Tensor, tpf: int, base_scale: float = 0.25, mapper: str = "linear",
             grid_h: int = 0, img_feat: Optional[torch.Tensor] = None, want_scores: bool = False,
             gather: bool = True, tail: Optional[torch.Tensor] = None,
             stats_ws: Optional[torch.Tensor] = None, score_dtype: Optional[torch.dtype] = None,
             newline: Optional[torch.Tensor] = None, params: Optional[PassParams] = None) -> CompressionResult:
    """One whole pass: feature tensor resident in HBM -> kept rows + indices + budgets.
    newline (mapper "grid_vid", INSTEAD of img_feat): the model's `image_newline` embedding, [D] or [1, D] in the input's
    dtype.  `rows` is then bit for bit `img_feat[global_idx]` for the img_feat LLaVA-Video's add_token_per_grid builds from
    `flattened_feat` and that vector -- without building it: the gather reads the kept rows from `flattened_feat` and
    writes the vector into the newline slots (vidcom2.py:93-96, :105-115).  Indices, K and budgets are unchanged.
    score_dtype: the dtype the pass scores in.  None or the input's dtype: the reference's behaviour (every op rounds to the
    input dtype).  torch.float32 over a bf16 / fp16 tensor: the reference applied to `flattened_feat.float()` -- the kept set
    a user gets today from `compress(x.float(), ...)` -- from the 16-bit tensor itself: no fp32 copy, half the bytes, rows
    gathered in the input dtype; `v_score` / `f_score` are then fp32 and `_ffi.set_mode` changes nothing, as for fp32 inputs.
    params: channel ratio, softmax temperature and Gaussian scales other than the reference's (PassParams); None, or a
    PassParams equal to the defaults: the reference's.
    tail ([m, D], e.g. LLaVA's newline embedding): written behind the kept rows by the gather launch itself;
    `rows` is then [K + m, D].  stats_ws: the workspace `fused.pool_stats` returned together with THIS tensor --
    the pass then skips its first sweep.
    Autograd: `rows` is differentiable (vidcom2_amd/autograd.py) with respect to the gathered-from tensor
    (`flattened_feat`, or `img_feat` for grid_vid -- flattened_feat then gets none, as in the reference; with `newline`
    both `flattened_feat` and `newline`, as through the stream built from them) and `tail`; indices, budgets and scores are
    not."""
    if isinstance(newline, PassParams) and params is None:
        # (`newline` took the twelfth position, which was `params`' before it existed: a PassParams handed over
        #  positionally still means what it meant)
        params, newline = newline, None
    if newline is not None:               # (argument errors first: nothing has touched the device yet)
        if mapper != "grid_vid":
            raise ValueError(f"newline is the grid_vid mapper's newline vector; got mapper={mapper!r}")
        if img_feat is not None:
            raise ValueError("give either img_feat or newline for grid mapping, not both")
    params = _norm_params(params)
    x = _prep(flattened_feat, "flattened_feat")
    score_dtype = _norm_score_dtype(score_dtype, x.dtype)
    if x.dim() != 2:
        raise RuntimeError(f"flattened_feat must be 2-D [frames*tokens, dim], got {tuple(x.shape)}")
    R, D = x.shape
    tpf = int(tpf)
    _c_params(params, D)                  # (the limits of the channel count, before the shape's own errors)
    if tpf <= 0 or R % tpf != 0:
        # the reference fails in frames = x.view(-1, tpf, C) (vidcom2.py:47)
        C = int(D * 0.5) if params is None else params.channels(D)
        raise RuntimeError(f"shape '[-1, {tpf}, {C}]' is invalid for input of size {R * C}")
    src = None
    nl = None
    if mapper == "grid_vid" and newline is not None:
        nl = _prep_newline(newline, D, x.dtype, x.device)
    elif mapper == "grid_vid":
        if img_feat is None:
            raise ValueError("img_feat required for grid mapping")
        src = _prep(img_feat, "img_feat")
        if src.dtype != x.dtype or src.shape[-1] != D:
            raise RuntimeError("img_feat must have the dtype and feature dim of flattened_feat")
        need = (R // tpf) * int(grid_h) * (int(grid_h) + 1)
        if src.dim() != 2 or src.shape[0] < need:
            # the reference fails in img[_map_grid_vid(...)] (vidcom2.py:96) with an IndexError
            raise IndexError(f"index {need - 1} is out of bounds for dimension 0 with size {src.shape[0]}"
                             if src.dim() == 2 else "img_feat must be 2-D [rows, dim]")
    tail_user = tail
    if tail is not None:
        tail = _prep(tail if tail.dim() == 2 else tail[None], "tail")
    if stats_ws is not None and (getattr(stats_ws, "_vc2_stats_for", None) != (R // tpf, tpf, D, x.dtype, x.data_ptr())
                                 or stats_ws.numel() < _ffi.workspace_bytes(R // tpf, tpf, D, x.dtype)):
        # another tensor (a copy was made), another (frames, tokens per frame) split -- e.g. a tpf that is not the
        # pooled grid -- or a workspace of unknown origin: its partials are not this call's, sweep 1 runs again
        stats_ws = None
    ntail = 0 if tail is None else tail.shape[0]
    if stats_ws is not None:          # (the statistics live in the caller's workspace: a plan around it, not cached)
        plan = CompressPlan(R // tpf, tpf, D, x.dtype, x.device, base_scale, mapper, grid_h, want_scores, gather,
                            tail_rows=ntail, ws=stats_ws, params=params, score_dtype=score_dtype)
    else:
        plan = _cached_plan(R // tpf, tpf, D, x.dtype, x.device, base_scale, mapper, grid_h, want_scores, gather, ntail,
                            fresh_outputs=True, params=params, score_dtype=score_dtype)
    plan.enqueue(x, src, tail, have_stats=stats_ws is not None, mirror=_EARLY_COUNT, newline=nl)
    if stats_ws is None and _PREALLOC and _PLAN_CACHE_MAX > 0 and plan.output_bytes() <= _SPARE_MAX_BYTES:
        plan.prepare_spare()              # (the GPU is busy for the next ~190 us: the next call's outputs cost nothing here)
    res = plan.finish()
    _check_budgets(res.ks, tpf, plan.arith_dtype)        # (RN_T(scale * N) rounds in the dtype the pass scores in)
    if nl is not None:
        if gather and _ag.wants_grad(flattened_feat, newline, tail_user):
            res.rows = _ag.attach_rows_grid(res.rows, flattened_feat, newline, res.global_idx, res.K, R // tpf, int(grid_h),
                                            tail=tail_user)
        return res
    gsrc = img_feat if mapper == "grid_vid" else flattened_feat
    if gather and _ag.wants_grad(gsrc, tail_user):
        res.rows = _ag.attach_rows([res.rows], [gsrc], res.global_idx, res.K, tail=tail_user)[0]
    return res


_LANES = threading.local()              # per thread: {device index: [streams]}


def _lane_streams(dev: torch.device, n: int):
    """The n extra streams compress_batch runs clips on -- created once per (thread, device) and kept for as long as the
    thread lives: the plan cache is keyed by stream, so fresh streams per call meant fresh plans (and workspaces) per
    call: 0.5-1.2 ms of set-up per batch."""
    by_dev = _LANES.__dict__.setdefault("by_dev", {})
    lst = by_dev.setdefault(dev.index if dev.index is not None else torch.cuda.current_device(), [])
    while len(lst) < n:
        lst.append(torch.cuda.Stream(dev))
    return lst[:n]


BATCH_LANES = 3          # compress_batch's default: clips in flight (16 cfg5 clips: 254 / 216 / 203 / 197 us per clip with 1 / 2 / 3 / 4)


def compress_batch(clips, tpf: int, base_scale: float = 0.25, in_flight: int = BATCH_LANES, gather: bool = True,
                   own_storage: bool = False, score_dtype: Optional[torch.dtype] = None,
                   params: Optional[PassParams] = None):
    """Compress several clips (a list of [F_i * tpf, D] tensors) with up to `in_flight` of them running
    concurrently, one HIP stream each.  A single pass leaves the GPU idle during its single-workgroup selection
    replays; further clips in flight fill those gaps (DESIGN.md "clips in flight"; every lane keeps a plan = a workspace).
    Returns one CompressionResult per clip, in order.  The reference has no batched form: its harness loops
    over clips (lmms-eval, batch size 1 per rank).
    `tpf` may also be a sequence of one tokens-per-frame value per clip (videos of different grids).
    params: one PassParams for every clip of the batch (None: the reference's hyper-parameters).
    score_dtype: as in `compress`, for every clip of the batch.
    Storage: for clips of ONE shape every result is a VIEW into batch-wide buffers (one allocation per output kind), so
    keeping any clip's rows / indices alive keeps the whole batch's buffers alive (n * capacity * D elements);
    own_storage=True hands every clip its own tensors instead (one extra device copy of the kept rows).
    Autograd: every clip's rows are differentiable with respect to that clip (vidcom2_amd/autograd.py)."""
    clips = list(clips)
    params = _norm_params(params)
    if _ag.wants_grad(*clips):
        return [_attach_clip(r, c) for r, c in zip(_compress_batch(clips, tpf, base_scale, in_flight, gather, own_storage,
                                                                   params, score_dtype), clips)]
    return _compress_batch(clips, tpf, base_scale, in_flight, gather, own_storage, params, score_dtype)


def _attach_clip(res: CompressionResult, clip: torch.Tensor) -> CompressionResult:
    if res.rows is not None and _ag.wants_grad(clip):
        res.rows = _ag.attach_rows([res.rows], [clip], res.global_idx, res.K)[0]
    return res


def _compress_batch(clips, tpf, base_scale: float, in_flight: int, gather: bool, own_storage: bool,
                    params: Optional[PassParams] = None, score_dtype: Optional[torch.dtype] = None):
    clips = [_prep(c, "clip") for c in clips]
    if not clips:
        return []
    dev = clips[0].device
    if isinstance(tpf, (list, tuple)):
        if len(tpf) != len(clips):
            raise ValueError(f"{len(tpf)} tokens-per-frame values for {len(clips)} clips")
        tpfs = [int(t) for t in tpf]
    else:
        tpfs = [int(tpf)] * len(clips)
    for i, (x, t) in enumerate(zip(clips, tpfs)):
        if x.dim() != 2 or t <= 0 or x.shape[0] % t != 0:
            raise RuntimeError(f"clip {i}: shape {tuple(x.shape)} is not [frames * {t}, dim]")
        _c_params(params, x.shape[1])      # (the channel count's limits, before anything is enqueued for any clip)
        _norm_score_dtype(score_dtype, x.dtype)
    cur = torch.cuda.current_stream(dev)
    lanes = [cur] + _lane_streams(dev, max(1, min(int(in_flight), len(clips))) - 1)
    plans = {}

    def plan_on(j, x, t):                 # lane j's cached plan for x's shape (its workspace: work on a stream is ordered)
        key = (j, x.shape, x.dtype, t)
        if key not in plans:
            with torch.cuda.stream(lanes[j]):
                plans[key] = _cached_plan(x.shape[0] // t, t, x.shape[1], x.dtype, dev, base_scale, "linear", 0, False,
                                          gather, 0, params=params, score_dtype=score_dtype)
        return plans[key]

    # Clips of one shape (the batched-eval case, BASELINE config 5): ONE allocation per output kind for the whole batch --
    # each clip's pass writes its slice -- on the caller's stream.  Round 4 looked a plan up, allocated six tensors and
    # recorded them on the caller's stream PER CLIP: ~100 us of host work per clip, more than the 75 us a lane's share of
    # the GPU time leaves -- 16 clips took 5.8 ms, slower than one at a time.
    same = all(c.shape == clips[0].shape and c.dtype == clips[0].dtype and c.device == dev for c in clips) \
        and all(t == tpfs[0] for t in tpfs)
    batch = plan_on(0, clips[0], tpfs[0])._alloc_outputs(len(clips)) if same else None
    for st in lanes[1:]:
        st.wait_stream(cur)               # inputs and the batch's buffers belong to the caller's stream
    outs = []
    for i, (x, t) in enumerate(zip(clips, tpfs)):
        j = i % len(lanes)
        plan = plan_on(j, x, t)
        if batch is not None:
            # (no record_stream on the batch's buffers: every lane is joined into the caller's stream below, before this
            #  function returns -- whatever the caller does with them, freeing included, is ordered behind the lanes' work)
            out = OutputSet(*(None if b is None else b[i] for b in batch))
        else:
            with torch.cuda.stream(lanes[j]):     # fresh per clip, allocated (and owned) on the lane's stream ...
                out = plan._alloc_outputs()
            if j:                                 # ... and consumed on the caller's
                for tn in out:
                    if tn is not None:
                        tn.record_stream(cur)
        plan.enqueue(x, stream=lanes[j], out=out)
        outs.append(out)
    for st in lanes[1:]:
        cur.wait_stream(st)               # results are safe to use on the current stream
    words = (batch.kout if batch is not None else torch.stack([o.kout for o in outs])).tolist()   # the single host sync
    res = [o.result(K, status) for o, (K, status) in zip(outs, words)]
    if batch is not None:
        _check_budgets(batch.ks, tpfs[0], plan_on(0, clips[0], tpfs[0]).arith_dtype)
        if own_storage:
            res = [CompressionResult(None if r.rows is None else r.rows.clone(), r.global_idx.clone(), r.ks.clone(), r.K)
                   for r in res]
    else:
        for r, t, x in zip(res, tpfs, clips):
            _check_budgets(r.ks, t, x.dtype if _norm_score_dtype(score_dtype, x.dtype) is None else torch.float32)
    return res


@_guarded
def vidcom2_compression(flattened_feat: torch.Tensor, model: str = "llava_ov", base_scale: float = 0.25,
                        frame_token_len: Optional[int] = None,
                        img_feat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reference: vidcom2.py:15-36.  Returns the gathered kept rows ([K, D], input dtype)."""
    if model not in MODEL_SPECS:
        raise ValueError(f"Unknown model: {model}")
    spec = MODEL_SPECS[model]
    tpf = frame_token_len if model in _DYNAMIC_TPF else spec["tpf"]
    if tpf is None:
        raise ValueError(f"frame_token_len required for {model}")
    tpf = _as_int(tpf)
    if spec["mapper"] == "grid_vid":
        if img_feat is None:
            # the reference scores first and raises in map_features (vidcom2.py:94); same exception
            raise ValueError("img_feat required for grid mapping")
        return compress(flattened_feat, tpf, base_scale, "grid_vid", spec["grid"], img_feat).rows
    return compress(flattened_feat, tpf, base_scale, "linear").rows


# ---------------------------------------------------------------------------------------------
# stage functions (same decomposition as the reference)
# ---------------------------------------------------------------------------------------------

@_guarded
def _channel_variance(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """x.var(dim=0, unbiased=False) (vidcom2.py:40): returns (var in T, fp32-widened copy)."""
    R, D = x.shape
    ws = _ffi.workspace(1, R, D, x.dtype, x.device)
    var_T = torch.empty(D, dtype=x.dtype, device=x.device)
    var_f = torch.empty(D, dtype=torch.float32, device=x.device)
    check(lib().vc2_chan_var(ptr(x), R, D, DTYPE_CODE[x.dtype], ptr(ws), ws.numel(), ptr(var_T), ptr(var_f),
                             stream_ptr(x.device)), "vc2_chan_var")
    return var_T, var_f


@_guarded
def low_var_channel_order(x: torch.Tensor, ratio: float = 0.5) -> torch.Tensor:
    """Indices torch.topk(var, int(D*ratio), largest=False) returns on the CPU reference, in ITS order
    (ascending variance, libstdc++ nth_element + sort tie order), replayed on the device
    (k_chan_select + k_chan_order: workgroup-parallel introselect + introsort)."""
    x = _prep(x, "x")
    D = x.shape[-1]
    k = int(D * ratio)
    _, var_f = _channel_variance(x)
    order = torch.empty(max(k, 1), dtype=torch.int32, device=x.device)
    perm = torch.empty(max(k, 1), dtype=torch.int32, device=x.device)
    if k > 0:
        check(lib().vc2_chan_select(ptr(var_f), D, k, None, None, ptr(perm), ptr(order), None, None,
                                    stream_ptr(x.device)), "vc2_chan_select")
    return order[:k].to(torch.int64)


@_guarded
def select_low_var_channels(x: torch.Tensor, ratio: float = 0.5) -> torch.Tensor:
    """Reference: vidcom2.py:38-43.  Returns x[:, idx] -- a copy, columns in topk order (differentiable w.r.t. x)."""
    x_user = x
    x = _prep(x, "x")
    if x.dim() != 2:
        raise RuntimeError("select_low_var_channels expects a 2-D [tokens, dim] tensor")
    idx = low_var_channel_order(x, ratio)
    R, D = x.shape
    C = idx.numel()
    out = torch.empty((R, C), dtype=x.dtype, device=x.device)
    if R and C:
        check(lib().vc2_gather_cols(ptr(x), R, D, DTYPE_CODE[x.dtype], ptr(idx), C, ptr(out), stream_ptr(x.device)),
              "vc2_gather_cols")
    if C and _ag.wants_grad(x_user):
        out = _ag.attach_cols(out, x_user, idx)
    return out


@_guarded
def compute_gaussian_scores(x: torch.Tensor, tpf: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference: vidcom2.py:45-57.  x = channel-selected features [F*tpf, C]; returns (v, f) [F, tpf]."""
    x = _prep(x, "x")
    tpf = _as_int(tpf)
    R, C = x.shape
    if tpf <= 0 or R % tpf != 0:
        raise RuntimeError(f"shape '[-1, {tpf}, {C}]' is invalid for input of size {R * C}")
    F = R // tpf
    ws = _ffi.workspace(F, tpf, C, x.dtype, x.device)
    v = torch.empty((F, tpf), dtype=x.dtype, device=x.device)
    f = torch.empty((F, tpf), dtype=x.dtype, device=x.device)
    check(lib().vc2_scores(ptr(x), F, tpf, C, DTYPE_CODE[x.dtype], None, C, None, ptr(ws), ws.numel(), ptr(v),
                           ptr(f), None, None, stream_ptr(x.device)), "vc2_scores")
    return v, f


def _multi_scale_gaussian(x: torch.Tensor, center: torch.Tensor, alphas: List[float]) -> torch.Tensor:
    """Reference: vidcom2.py:59-62.  x T[F, N, C], center T[1, 1, C] or T[F, 1, C] (the two shapes
    compute_gaussian_scores uses, vidcom2.py:51-52) -> T[F, N].  The fused pass never calls this (it
    does not materialise x); it exists for callers of the helper itself."""
    alphas = [float(a) for a in alphas]
    if not alphas:
        return 0                     # Python's sum() over no terms, exactly like the reference
    # (x - center) broadcasts like torch: any x [..., C] and any center broadcastable to it
    out_shape = torch.broadcast_shapes(tuple(x.shape), tuple(center.shape))
    if len(out_shape) < 1:
        raise RuntimeError("_multi_scale_gaussian: x must have a channel dimension")
    C = out_shape[-1]
    xb = x.expand(out_shape)
    cb = center.to(x.dtype).expand(out_shape)
    lead = out_shape[:-1]
    R = 1
    for d in lead:
        R *= int(d)
    # centre layouts the kernel knows: one row, one row per "frame" (constant along the last leading dim), or one
    # row per token (anything else)
    if all(int(cb.stride(i)) == 0 or out_shape[i] == 1 for i in range(len(lead))):
        F, N, cc = 1, R, cb[tuple(0 for _ in lead)].reshape(1, C)
    elif len(lead) >= 2 and (int(cb.stride(len(lead) - 1)) == 0 or out_shape[len(lead) - 1] == 1):
        N = int(out_shape[len(lead) - 1])
        F = R // N
        cc = cb.select(len(lead) - 1, 0).reshape(F, C)
    else:
        F, N, cc = R, 1, cb.reshape(R, C)
    xx = _prep(xb.reshape(R, C), "x")
    cc = _prep(cc, "center")
    out = torch.empty(lead, dtype=x.dtype, device=x.device)
    if R == 0:
        return out
    arr = (ctypes.c_double * len(alphas))(*alphas)
    with on_device(x.device):
        check(lib().vc2_multi_scale_gaussian(ptr(xx), F, N, C, DTYPE_CODE[x.dtype], ptr(cc), cc.shape[0], arr,
                                             len(alphas), ptr(out), stream_ptr(x.device)), "_multi_scale_gaussian")
    return out


@_guarded
def compute_scales(scores: torch.Tensor, base: float, temp: float = 0.01) -> torch.Tensor:
    """Reference: vidcom2.py:64-68.  scores T[F] -> scales T[F]."""
    s = _prep(scores, "scores")
    if s.dim() != 1:
        raise RuntimeError("compute_scales expects a 1-D tensor of per-frame scores")
    F = s.numel()
    out = torch.empty_like(s)
    if F == 0:
        return out
    ws = torch.empty(3 * (F * 4 + 256), dtype=torch.uint8, device=s.device)
    check(lib().vc2_compute_scales(ptr(s), F, float(base), float(temp), DTYPE_CODE[s.dtype], ptr(ws), ws.numel(),
                                   ptr(out), stream_ptr(s.device)), "vc2_compute_scales")
    return out


def _select(scores: torch.Tensor, scales: torch.Tensor, tpf: int, map_mode: int, grid_h: int = 0):
    sc = _prep(scores, "scores")
    sl = _prep(scales, "scales")
    if sc.dim() != 2 or sl.dim() != 1 or sl.numel() != sc.shape[0]:
        raise RuntimeError("scores must be [F, N] and scales [F]")
    if sl.dtype != sc.dtype:
        sl = sl.to(sc.dtype)
    F, N = sc.shape
    extra = grid_h if map_mode == MAP_GRID_VID else 0
    cap = F * (N + extra)
    ws = torch.empty(F * N * 4 + F * 4 + 1024, dtype=torch.uint8, device=sc.device)
    ks = torch.empty(F, dtype=torch.int64, device=sc.device)
    offs = torch.empty(F + 1, dtype=torch.int64, device=sc.device)
    idx = torch.empty(cap, dtype=torch.int64, device=sc.device)
    kout = torch.empty(2, dtype=torch.int64, device=sc.device)
    with on_device(sc.device):
        check(lib().vc2_select(ptr(sc), ptr(sl), F, N, int(tpf), DTYPE_CODE[sc.dtype], map_mode, grid_h, ptr(ws),
                               ws.numel(), ptr(ks), ptr(offs), ptr(idx), cap, ptr(kout), stream_ptr(sc.device)),
              "vc2_select")
    return idx, ks, offs, kout


def select_outlier_indices(scores: torch.Tensor, scales: torch.Tensor, tpf: int) -> List[torch.Tensor]:
    """Reference: vidcom2.py:70-78.  Returns F ascending int64 index tensors (one host sync, as the
    reference's ``.tolist()``)."""
    idx, ks, _, kout = _select(scores, scales, _as_int(tpf), MAP_LOCAL)
    host = torch.cat((ks, kout)).tolist()     # budgets + (count, status): still ONE host sync
    ks_host, (K, status) = host[:-2], host[-2:]
    if status:
        _raise_status(int(status), int(idx.numel()), int(K))
    N = scores.shape[1]
    if any(k > N for k in ks_host):          # ks = round(scales * tpf) with tpf > N: torch.topk's own error (vidcom2.py:76)
        raise RuntimeError("selected index k out of range")
    return list(torch.split(idx[: sum(ks_host)], ks_host))


def _cat_indices(indices: List[torch.Tensor]):
    if len(indices) == 0:
        raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
    dev = indices[0].device
    require_device(indices[0], "indices[0]")
    ks_host = [int(i.numel()) for i in indices]
    loc = torch.cat([i.to(torch.int64) for i in indices]).contiguous()
    ks = torch.tensor(ks_host, dtype=torch.int64)
    offs = torch.zeros(len(indices) + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(ks, 0)
    return loc, ks.to(dev), offs.to(dev), ks_host


@_guarded
def _map_linear_offset(indices: List[torch.Tensor], tpf: int) -> torch.Tensor:
    """Reference: vidcom2.py:99-103."""
    loc, ks, offs, _ = _cat_indices(indices)
    out = torch.empty_like(loc)
    if loc.numel():
        check(lib().vc2_map_indices(ptr(loc), ptr(ks), ptr(offs), len(indices), MAP_LINEAR, _as_int(tpf), ptr(out),
                                    stream_ptr(loc.device)), "vc2_map_indices")
    return out


@_guarded
def _map_grid_vid(indices: List[torch.Tensor], h: int) -> torch.Tensor:
    """Reference: vidcom2.py:105-115 (per frame: kept tokens on the h x (h+1) grid, then its h newlines)."""
    loc, ks, offs, ks_host = _cat_indices(indices)
    h = _as_int(h)
    out = torch.empty(loc.numel() + len(indices) * h, dtype=torch.int64, device=loc.device)
    check(lib().vc2_map_indices(ptr(loc), ptr(ks), ptr(offs), len(indices), MAP_GRID_VID, h, ptr(out),
                                stream_ptr(loc.device)), "vc2_map_indices")
    return out


@_guarded
def _gather_rows(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    src_user = src
    src = _prep(src, "features")
    K = idx.numel()
    out = torch.empty((K,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    if K == 0:
        return _ag.attach_rows([out], [src_user], idx, 0)[0] if _ag.wants_grad(src_user) else out
    D = src[0].numel()
    kdev = torch.tensor([K, 0], dtype=torch.int64, device=src.device)
    check(lib().vc2_gather_rows(ptr(src), src.shape[0], D, DTYPE_CODE[src.dtype], ptr(idx), ptr(kdev), K, ptr(out),
                                stream_ptr(src.device)), "vc2_gather_rows")
    if _ag.wants_grad(src_user):
        # (a caller's index list: the backward checks it for duplicates and then accumulates like torch)
        out = _ag.attach_rows([out], [src_user], idx, K, validate=True)[0]
    return out


def _gather_rows_grid(flat: torch.Tensor, idx: torch.Tensor, newline: torch.Tensor, F: int, h: int) -> torch.Tensor:
    """rows idx[] (grid index space) of the [F*h*(h+1), D] stream made of `flat` [F*h*h, D] and the newline vector."""
    flat_user = flat
    flat = _prep(flat, "features")
    if flat.dim() != 2 or flat.shape[0] != F * h * h:
        raise RuntimeError(f"features must be [{F} * {h} * {h}, dim] for {F} frames on a {h} x {h} grid, got "
                           f"{tuple(flat.shape)}")
    D = flat.shape[1]
    nl = _prep_newline(newline, D, flat.dtype, flat.device)
    K = idx.numel()
    out = torch.empty((K, D), dtype=flat.dtype, device=flat.device)
    if K:
        check(lib().vc2_gather_rows_grid(ptr(flat), F, h, D, DTYPE_CODE[flat.dtype], ptr(idx), None, K, ptr(nl), ptr(out),
                                         stream_ptr(flat.device)), "vc2_gather_rows_grid")
    if _ag.wants_grad(flat_user, newline):
        out = _ag.attach_rows_grid(out, flat_user, newline, idx, K, F, h, validate=True)
    return out


@_guarded
def map_features(indices: List[torch.Tensor], flat: torch.Tensor, img: Optional[torch.Tensor],
                 spec: Dict[str, Any], *, newline: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Reference: vidcom2.py:80-97.  newline (a grid_vid spec, with img None): the model's [D] newline embedding -- the rows
    of the stream add_token_per_grid would build from `flat` and it, gathered without building it (vc2_gather_rows_grid)."""
    if spec["mapper"] == "linear":
        stride = flat.shape[0] // len(indices)                     # vidcom2.py:89
        return _gather_rows(flat, _map_linear_offset(indices, stride))
    elif spec["mapper"] == "grid_vid":
        if img is None and newline is not None:
            return _gather_rows_grid(flat, _map_grid_vid(indices, spec["grid"]), newline, len(indices), int(spec["grid"]))
        if img is None:
            raise ValueError("img_feat required for grid mapping")
        if newline is not None:
            raise ValueError("give either img or newline for grid mapping, not both")
        return _gather_rows(img, _map_grid_vid(indices, spec["grid"]))
    return flat

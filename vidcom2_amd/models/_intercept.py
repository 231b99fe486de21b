"""Plumbing shared by the model hooks.

The reference's hooks (token_compressor/vidcom2/models/*.py) are whole-function copies of upstream
LLaVA-NeXT / HF transformers methods with one or two inserted calls into the compression pass.
The hooks here are *wrappers* instead: they run the model class's own, unmodified method and
intercept the two or three attributes on the instance that bracket the insertion point.  They
therefore follow whatever upstream version is installed and carry no upstream code.

`shadow(obj, name=value, ...)` puts `value` into the instance `__dict__` for the duration of a
`with` block.  An instance-dict entry wins over class functions (non-data descriptors) and over
`nn.Module` sub-modules / parameters (those are only reached through `__getattr__`), so no module
state is touched and everything is restored on exit, also when the wrapped call raises.
"""
from __future__ import annotations

import contextlib
import os
from typing import Any, Callable

_MISSING = object()


@contextlib.contextmanager
def shadow(obj: Any, **attrs: Any):
    saved = {}
    d = obj.__dict__
    try:
        for name, value in attrs.items():
            saved[name] = d.get(name, _MISSING)
            d[name] = value
        yield
    finally:
        for name, old in saved.items():
            if old is _MISSING:
                d.pop(name, None)
            else:
                d[name] = old


def original_method(obj: Any, name: str, hook: Callable) -> Callable:
    """The class's own `name`, bound to `obj` -- i.e. what ran before `hook` was installed with
    `types.MethodType(hook, obj)` (README.md:76-83 of the reference) or assigned on a subclass."""
    for klass in type(obj).__mro__:
        fn = klass.__dict__.get(name)
        if fn is None:
            continue
        if getattr(fn, "__func__", fn) is hook:
            continue
        return fn.__get__(obj, type(obj))
    raise AttributeError(f"{type(obj).__name__} has no original '{name}' to wrap "
                         "(the hook must be installed on a model that defines it)")


def retention_ratio() -> float:
    """`R_RATIO` env knob, default 0.25 (models/llava.py:124, models/qwen2_5_vl.py:135)."""
    return float(os.getenv("R_RATIO", "0.25"))


def _float_knob(name: str):
    raw = os.getenv(name)
    if raw is None:
        return None
    try:
        return float(raw)
    except ValueError:
        raise ValueError(f"{name}={raw!r}: expected a number") from None


def pass_params():
    """`VC2_CHANNEL_RATIO` (float), `VC2_TEMP` (float) and `VC2_ALPHAS` (comma-separated floats), read at call time: the
    hyper-parameters the reference fixes in its stage functions' defaults (vidcom2.py:38, :54, :64), as the `PassParams`
    the hooks hand to `compress` / `compress_batch`.  None when none of them is set -- the hooks' call is then the one
    without params; an unset knob keeps the reference's value.  A malformed or out-of-range value raises ValueError
    naming the knob."""
    from ..vidcom2 import PassParams
    ratio, temp, raw = _float_knob("VC2_CHANNEL_RATIO"), _float_knob("VC2_TEMP"), os.getenv("VC2_ALPHAS")
    if ratio is None and temp is None and raw is None:
        return None
    kw = {}
    if raw is not None:
        try:
            kw["alphas"] = tuple(float(a) for a in raw.split(","))
        except ValueError:
            raise ValueError(f"VC2_ALPHAS={raw!r}: expected comma-separated numbers") from None
    if ratio is not None:
        kw["channel_ratio"] = ratio
    if temp is not None:
        kw["temp"] = temp
    for knob, key in (("VC2_CHANNEL_RATIO", "channel_ratio"), ("VC2_TEMP", "temp"), ("VC2_ALPHAS", "alphas")):
        if key in kw:                                    # each knob checked on its own, so that the error can name it
            try:
                PassParams(**{key: kw[key]})
            except ValueError as e:
                raise ValueError(f"{knob}={os.getenv(knob)!r}: {e}") from None
            except NotImplementedError as e:
                raise NotImplementedError(f"{knob}={os.getenv(knob)!r}: {e}") from None
    return PassParams(**kw)


def score_dtype():
    """`VC2_SCORE_DTYPE=fp32`, read at call time: the hooks' passes score bf16 / fp16 features in fp32 (the reference applied
    to the widened features, `compress(..., score_dtype=torch.float32)`; a no-op for fp32 features).  None when unset;
    any other value raises ValueError naming the knob."""
    raw = os.getenv("VC2_SCORE_DTYPE")
    if raw is None:
        return None
    if raw != "fp32":
        raise ValueError(f"VC2_SCORE_DTYPE={raw!r}: the only value is 'fp32' (unset: score in the features' dtype)")
    import torch
    return torch.float32


def params_kwargs() -> dict:
    """The knobs' keyword arguments for the hooks' calls into the pass -- `params` (pass_params()) and `score_dtype`
    (score_dtype()) --, each only when its knobs are set: with none set the call is exactly the one without them."""
    kw = {}
    p = pass_params()
    if p is not None:
        kw["params"] = p
    sd = score_dtype()
    if sd is not None:
        kw["score_dtype"] = sd
    return kw


def grid_newline_enabled() -> bool:
    """`VC2_GRID_NEWLINE` env knob, `on` by default, read at call time: LLaVA-Video's grid hook gathers the kept rows from
    the pooled features and the model's `image_newline` vector instead of building the newline stream with the model's
    `add_token_per_grid` (same result, bit for bit).  `off`: the model's own method builds the stream, as before."""
    raw = os.getenv("VC2_GRID_NEWLINE", "on")
    if raw not in ("on", "off"):
        raise ValueError(f"VC2_GRID_NEWLINE={raw!r}: expected 'on' or 'off'")
    return raw == "on"


def compressor_enabled() -> bool:
    """`COMPRESSOR=vidcom2` env knob (models/qwen2_5_vl.py:121)."""
    return os.getenv("COMPRESSOR") == "vidcom2"


def batched_prefill_enabled() -> bool:
    """`VC2_BATCHED_PREFILL=1` env knob: the Qwen-VL hooks also prune video prefills of batch size > 1 (the reference
    leaves those unpruned, models/qwen2_5_vl.py:120-130)."""
    return os.getenv("VC2_BATCHED_PREFILL") == "1"

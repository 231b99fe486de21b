"""CPU: the fp32-scored pass over 16-bit inputs (`score_dtype=torch.float32`) -- its fixture is pinned to the reference
through the CPU oracle on the widened input, and its surface exists: the ABI entry point, the Python argument, the
hooks' knob."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, synth
from vidcom2_amd.models import _intercept as I

import _score_dtype as SD
from conftest import ROOT

CASES = SD.load()


@pytest.fixture(autouse=True)
def _mode():
    O.set_mode("exact")
    yield
    O.set_mode("torch")


def test_fixture_covers_what_it_must():
    """Every shape of the candidate list in both storage dtypes, the grid_vid case, k = 1, k = N, the two cases with
    non-default hyper-parameters; at least 90 % of the candidates admitted, each with the admission margin."""
    cands = SD.candidates()
    assert len(CASES) >= 0.9 * len(cands)
    ids = {SD.case_id(c) for c in CASES}
    assert ids <= {SD.case_id(c) for c in cands}
    for shape in SD.SHAPES:
        for dt in ("bf16", "f16"):
            assert any((c["F"], c["N"], c["D"]) == shape and c["dtype"] == dt and c["mapper"] == "linear" for c in CASES)
    assert any(c["mapper"] == "grid_vid" for c in CASES)
    assert any(c["ks"] == [1] for c in CASES) and any(c["ks"] == [c["N"]] and c["F"] == 1 for c in CASES)
    assert sum(SD.has_params(c) for c in CASES) == 2
    for c in CASES:
        assert c["margin"] is None or c["margin"] >= SD.MARGIN_MIN
        assert 0.0 <= c["native_overlap"] <= 1.0


@pytest.mark.parametrize("c", CASES, ids=SD.case_id)
def test_oracle_reproduces_the_reference_on_the_widened_input(c):
    x = SD.make_input(c)
    assert synth.sha256_tensor(x) == c["x_sha256"]
    o = SD.oracle_pass(x.float(), c)
    assert o["ks"] == c["ks"]
    gidx = SD.grid_indices(o["keep"], o["ks"], c) if c["mapper"] == "grid_vid" else o["keep"]
    assert gidx.tolist() == c["global_idx"]
    assert o["v"].dtype == torch.float32
    dv = np.abs(np.asarray(o["v"][0, :16].tolist()) - np.asarray(c["v_head"])).max()
    df = np.abs(np.asarray(o["f"][0, :16].tolist()) - np.asarray(c["f_head"])).max()
    assert dv <= SD.SCORE_TOL and df <= SD.SCORE_TOL, (dv, df)


def test_ex4_is_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vc2.h")).read(), flags=re.S)
    m = re.search(r"int\s+vc2_compress_ex4\s*\(([^;]*)\)\s*;", src)
    assert m, "vc2_compress_ex4 is not declared in include/vc2.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args[-2] == "int score_dtype" and args[-1] == "void* stream"
    ex3 = re.search(r"int\s+vc2_compress_ex3\s*\(([^;]*)\)\s*;", src).group(1).split(",")
    assert len(args) == len(ex3) + 1                     # ex3's arguments plus the score dtype
    assert hasattr(ctypes.CDLL(_ffi.LIB_PATH), "vc2_compress_ex4")
    assert "vc2_compress_ex4" in _ffi.EXPORTED_SYMBOLS
    assert len(_ffi._SIGNATURES["vc2_compress_ex4"]) == len(_ffi._SIGNATURES["vc2_compress_ex3"]) + 1


def test_python_signatures_carry_score_dtype():
    for fn in (vc.compress, vc.compress_batch, vc.vidcom2.CompressPlan.__init__):
        par = inspect.signature(fn).parameters
        assert "score_dtype" in par and par["score_dtype"].default is None
    # the reference's own signatures stay the reference's
    assert "score_dtype" not in inspect.signature(vc.vidcom2_compression).parameters


def test_score_dtype_is_normalised_and_validated_on_the_host():
    norm = vc.vidcom2._norm_score_dtype
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert norm(None, dt) is None and norm(dt, dt) is None
    assert norm(torch.float32, torch.bfloat16) is torch.float32 and norm(torch.float32, torch.float16) is torch.float32
    for sd, dt in ((torch.float16, torch.bfloat16), (torch.bfloat16, torch.float16), (torch.bfloat16, torch.float32),
                   (torch.float64, torch.bfloat16), ("fp32", torch.bfloat16)):
        with pytest.raises(ValueError, match="score_dtype"):
            norm(sd, dt)


@pytest.fixture
def knob(monkeypatch):
    for k in ("VC2_SCORE_DTYPE", "VC2_CHANNEL_RATIO", "VC2_TEMP", "VC2_ALPHAS"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_funnel_adds_nothing_when_the_knob_is_unset(knob):
    assert I.score_dtype() is None and I.params_kwargs() == {}


def test_funnel_hands_fp32_on(knob):
    knob.setenv("VC2_SCORE_DTYPE", "fp32")
    assert I.params_kwargs() == {"score_dtype": torch.float32}
    knob.setenv("VC2_TEMP", "0.5")                       # ... next to the other knobs' argument
    assert I.params_kwargs() == {"params": vc.PassParams(temp=0.5), "score_dtype": torch.float32}
    knob.delenv("VC2_SCORE_DTYPE")                       # read at call time
    assert I.params_kwargs() == {"params": vc.PassParams(temp=0.5)}


@pytest.mark.parametrize("value", ["fp64", "bf16", "float32", ""])
def test_funnel_refuses_any_other_value_by_name(knob, value):
    knob.setenv("VC2_SCORE_DTYPE", value)
    with pytest.raises(ValueError, match="VC2_SCORE_DTYPE"):
        I.params_kwargs()

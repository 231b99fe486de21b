"""CPU: the grid gather without the newline stream (vc2_gather_rows_grid, vc2_compress_ex5, `newline=` of compress /
CompressPlan.enqueue / map_features, the LLaVA-Video hook's route): the symbols are declared, exported and bound, the
Python API has the argument where it belongs and nowhere else, the argument errors come before any device access, and on
CPU tensors the hook still goes through the model's own add_token_per_grid.  The kernel itself: test_grid_newline_gpu."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

import _stub_models as S
import oracle as O
import vidcom2_amd as vc
from conftest import ROOT, load_json
from vidcom2_amd import _ffi, synth
from vidcom2_amd.vidcom2 import MODEL_SPECS, CompressPlan

NEW = ("vc2_gather_rows_grid", "vc2_compress_ex5")
ERR_ARG = -1


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "vc2.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", src), f"{name} is not declared in include/vc2.h"
        assert hasattr(lib, name) and name in _ffi.EXPORTED_SYMBOLS
    # vc2_compress_ex4's arguments plus `const void* newline` in front of the stream
    m = re.search(r"int\s+vc2_compress_ex5\s*\(([^;]*)\)\s*;", src)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args[-2] == "const void* newline" and args[-1] == "void* stream"
    assert len(_ffi._SIGNATURES["vc2_compress_ex5"]) == len(_ffi._SIGNATURES["vc2_compress_ex4"]) + 1 == len(args)
    m = re.search(r"int\s+vc2_gather_rows_grid\s*\(([^;]*)\)\s*;", src)
    names = [a.strip().split()[-1].lstrip("*") for a in m.group(1).replace("\n", " ").split(",")]
    assert names == ["src", "F", "h", "D", "dtype", "idx", "n_dev", "n_max", "newline", "out", "stream"]
    assert len(_ffi._SIGNATURES["vc2_gather_rows_grid"]) == len(names)
    assert "vidcom2.py:93-96" in src and "105-115" in src


def test_newline_is_a_parameter_where_it_belongs():
    for fn in (vc.compress, CompressPlan.enqueue, vc.map_features):
        p = inspect.signature(fn).parameters
        assert "newline" in p and p["newline"].default is None, fn
    assert inspect.signature(vc.map_features).parameters["newline"].kind is inspect.Parameter.KEYWORD_ONLY
    # the reference's signature, exactly (vidcom2.py:15)
    assert list(inspect.signature(vc.vidcom2_compression).parameters) == ["flattened_feat", "model", "base_scale",
                                                                         "frame_token_len", "img_feat"]


def test_params_in_the_twelfth_position_still_means_params():
    """`newline` stands where `params` stood for positional callers: a PassParams there is taken as params -- the call
    gets past the newline's argument checks (a newline with the linear mapper is a ValueError) to the device check."""
    from vidcom2_amd.vidcom2 import PassParams
    x = torch.zeros(2 * 9, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vc.compress(x, 9, 0.25, "linear", 0, None, False, True, None, None, None, PassParams(0.25))
    assert list(inspect.signature(vc.compress).parameters)[-1] == "params"


def _host(n=64):
    """A non-null pointer that is never dereferenced: every call below is refused on its arguments."""
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_c_argument_errors_come_before_any_device_access():
    L = _ffi.lib()
    p = _host()
    # the stage call: a null newline, a null source, a bad dtype / shape
    assert L.vc2_gather_rows_grid(p, 2, 3, 8, 1, p, None, 4, None, p, None) == ERR_ARG
    assert "null" in _ffi.last_error()
    assert L.vc2_gather_rows_grid(None, 2, 3, 8, 1, p, None, 4, p, p, None) == ERR_ARG
    for F, h, D, dt, n in ((0, 3, 8, 1, 4), (2, 0, 8, 1, 4), (2, 3, 0, 1, 4), (2, 3, 8, 3, 4), (2, 3, 8, 1, -1)):
        assert L.vc2_gather_rows_grid(p, F, h, D, dt, p, None, n, p, p, None) == ERR_ARG, (F, h, D, dt, n)

    def ex5(map_mode, grid_h, N, newline):
        return L.vc2_compress_ex5(p, 2, N, 8, 1, 0.25, map_mode, grid_h, None, 0, p, 64, p, p, 16, p, p, None, None, None, 0, 0,
                                  None, None, 1, newline, None)
    assert ex5(_ffi.MAP_LINEAR, 0, 9, p) == ERR_ARG                 # a newline pointer with another map mode
    assert "grid_vid" in _ffi.last_error()
    assert ex5(_ffi.MAP_LOCAL, 0, 9, p) == ERR_ARG
    assert ex5(_ffi.MAP_GRID_VID, 3, 10, p) == ERR_ARG              # h * h != N
    assert "grid_h" in _ffi.last_error()
    assert ex5(_ffi.MAP_GRID_VID, 0, 9, p) == ERR_ARG


def test_python_argument_errors_come_before_any_device_access():
    """CPU tensors: anything that reached the device path would raise the package's "no CPU fallback" RuntimeError."""
    x, nl, img = torch.zeros(2 * 9, 8), torch.zeros(8), torch.zeros(2 * 12, 8)
    with pytest.raises(ValueError, match="not both"):
        vc.compress(x, 9, 0.25, "grid_vid", 3, img, newline=nl)
    with pytest.raises(ValueError, match="grid_vid"):
        vc.compress(x, 9, 0.25, "linear", newline=nl)
    with pytest.raises(ValueError, match="grid_vid"):
        vc.compress(x, 9, 0.25, newline=nl)
    ind = [torch.arange(2), torch.arange(3)]
    with pytest.raises(ValueError, match="img_feat required for grid mapping"):      # as before
        vc.map_features(ind, x, None, dict(mapper="grid_vid", grid=3))
    with pytest.raises(TypeError):                                                    # keyword-only
        vc.map_features(ind, x, None, dict(mapper="grid_vid", grid=3), nl)
    with pytest.raises(TypeError):
        vc.vidcom2_compression(x, "llava_vid", newline=nl)


def test_the_knob(monkeypatch):
    from vidcom2_amd.models._intercept import grid_newline_enabled
    monkeypatch.delenv("VC2_GRID_NEWLINE", raising=False)
    assert grid_newline_enabled()
    monkeypatch.setenv("VC2_GRID_NEWLINE", "off")
    assert not grid_newline_enabled()
    monkeypatch.setenv("VC2_GRID_NEWLINE", "on")
    assert grid_newline_enabled()
    monkeypatch.setenv("VC2_GRID_NEWLINE", "maybe")
    with pytest.raises(ValueError, match="VC2_GRID_NEWLINE"):
        grid_newline_enabled()


@pytest.mark.parametrize("name", ["video_grid_bf16", "video_grid_f32_r50"])
def test_hook_on_cpu_tensors_still_builds_the_stream(name, monkeypatch):
    """CPU tensors take today's route whatever the knob says: the stub model's add_token_per_grid runs exactly once per
    video (the oracle stands in for the device pass, as in test_hooks), and the golden digest comes out."""
    import vidcom2_amd.models.llava as HL
    c = next(c for c in load_json("hook_cases.json")["llava"] if c["name"] == name)
    O.set_mode("torch")
    monkeypatch.setattr(HL, "vidcom2_compression",
                        lambda flat, model="llava_ov", base_scale=0.25, frame_token_len=None, img_feat=None:
                        O.vidcom2_compression(flat.contiguous(), model, base_scale, frame_token_len, img_feat))
    monkeypatch.setenv("R_RATIO", c["r"])
    monkeypatch.delenv("VC2_GRID_NEWLINE", raising=False)
    ids, feats = S.llava_inputs(c)
    calls = []

    class Counting(S.StubLlava):
        def add_token_per_grid(self, image_feature):
            calls.append(tuple(image_feature.shape))
            return super().add_token_per_grid(image_feature)

    m = Counting(c["D"], S.DT[c["dt"]], "cpu", c["seed"], c["merge"], c["newline"])
    m.prepare_inputs_labels_for_multimodal = types.MethodType(HL.cus_prepare_inputs_labels_for_multimodal, m)
    comp = m.prepare_inputs_labels_for_multimodal(ids, None, None, None, None, [feats], ["video"], None)
    assert calls == [(c["F"], MODEL_SPECS["llava_vid"]["tpf"], c["D"])]
    assert synth.sha256_tensor(comp[4]) == c["comp_sha"]
    assert "add_token_per_grid" not in m.__dict__ and "get_2dPool" not in m.__dict__

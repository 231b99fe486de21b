"""vc2_workspace_bytes is one size per shape (include/vc2.h): the numerics mode -- process-wide or a thread's override --
must not change it, so that a C caller who sized its workspace in one mode can run the pass in another.  (The ORD form's
block sums, o_bsum, used to be reserved only when the mode was a "torch order" one.)  Host arithmetic only: runs without
a GPU.  Also here, because it is host arithmetic as well: the `leftover` donor of tests/_guarded_ws.py has a workspace at
least as large as every shape the workspace-contract tests use, so that its bytes cover each of them."""
import pytest
import torch

import _guarded_ws as G
from vidcom2_amd import _ffi

TARGET = [(128, 196, 3584, torch.bfloat16), (128, 196, 3584, torch.float16), (128, 196, 3584, torch.float32)]
# shapes around the ORD form's conditions: D in {1024, 3584, 4096}, N <= 512, every frame workgroup resident
ORD_EDGES = [(8, 512, 4096, torch.bfloat16), (8, 513, 4096, torch.bfloat16), (448, 16, 1024, torch.float16),
             (449, 16, 1024, torch.float16), (512, 16, 1024, torch.bfloat16), (600, 16, 1024, torch.bfloat16),
             (8, 196, 2048, torch.bfloat16), (3, 15, 1024, torch.float16)]
SHAPES = sorted(set(G.SHAPES + TARGET + ORD_EDGES + [G.DONOR[:4]]), key=lambda s: (s[0] * s[1] * s[2], str(s)))


def sid(s):
    return f"{s[0]}x{s[1]}x{s[2]}-{str(s[3]).split('.')[-1]}"


@pytest.fixture(autouse=True)
def _restore_mode():
    yield
    assert _ffi.lib().vc2_set_thread_mode(-1) == 0
    _ffi.set_mode("torch")


@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_workspace_size_does_not_depend_on_the_mode(shape):
    L = _ffi.lib()
    F, N, D, dt = shape
    _ffi.set_mode("torch")
    want = _ffi.workspace_bytes(F, N, D, dt)
    assert want > 0
    for mode in (0, 1, 2, 3, 4):
        assert L.vc2_set_mode(mode) == 0 and L.vc2_get_mode() == mode
        assert _ffi.workspace_bytes(F, N, D, dt) == want, f"process-wide mode {mode}"
    assert L.vc2_set_mode(4) == 0
    for mode in (0, 1, 2, 3, 4):
        assert L.vc2_set_thread_mode(mode) == 0 and L.vc2_get_mode() == mode
        assert _ffi.workspace_bytes(F, N, D, dt) == want, f"thread override {mode}"
    assert L.vc2_set_mode(0) == 0                      # ... and an override on top of another process-wide mode
    assert L.vc2_set_thread_mode(4) == 0
    assert _ffi.workspace_bytes(F, N, D, dt) == want, "thread override 4 over process-wide 0"


def test_leftover_donor_covers_every_contract_shape():
    F, N, D, dt = G.DONOR[:4]
    donor = _ffi.workspace_bytes(F, N, D, dt)
    for s in G.SHAPES:
        assert _ffi.workspace_bytes(*s) <= donor, (sid(s), _ffi.workspace_bytes(*s), donor)

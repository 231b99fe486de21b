"""The options `compress` takes from the LLaVA hooks, in the chunked pass (vidcom2_amd/chunked.py), CPU side: the new
symbols are declared, exported and bound; the C entry points refuse bad arguments before any device access; the driver with
oracle-backed CPU stages injected -- the executable definition of the options -- equals the oracle on the concatenation
followed by _map_grid_vid / torch.cat; every argument error is raised with nothing built or enqueued.  The kernels:
test_chunked_options_gpu."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from conftest import ROOT
from vidcom2_amd import _ffi, chunked, synth

from _ragged_shards import RaggedOracleStages

NEW = ("vc2_gather_rows_grid_chunks", "vc2_select_chunks_x", "vc2_pool_stats_blocks")
ERR_ARG, ERR_UNSUPPORTED = -1, -3
OPTIONS = ("mapper", "grid_h", "newline", "tail", "want_scores")


# ---- 1. the symbols ------------------------------------------------------------------------------------------------------

def _declared(src, name):
    m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/vc2.h"
    args = re.sub(r"/\*.*?\*/", " ", m.group(1).replace("\n", " "))
    return [a.strip().split()[-1].lstrip("*") for a in args.split(",")]


def test_symbols_are_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "vc2.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name) and name in _ffi.EXPORTED_SYMBOLS
        assert len(_ffi._SIGNATURES[name]) == len(_declared(src, name)), name
    assert _declared(src, "vc2_gather_rows_grid_chunks") == [
        "chunks", "chunk_rows", "n_chunks", "h", "D", "dtype", "idx", "n_dev", "n_max", "newline", "tail", "tail_rows", "dst",
        "dst_rows", "status", "stream"]
    # vc2_select_chunks_o's arguments, then the mapping and the gather options
    x, o = _declared(src, "vc2_select_chunks_x"), _declared(src, "vc2_select_chunks_o")
    assert x == o + ["map_mode", "grid_h", "newline", "tail", "tail_rows"]
    assert _ffi._SIGNATURES["vc2_select_chunks_x"][:len(o)] == _ffi._SIGNATURES["vc2_select_chunks_o"]
    assert _declared(src, "vc2_pool_stats_blocks") == [
        "xin", "F", "H", "W", "D", "dtype", "mode", "F_total", "block_frames", "ws", "ws_bytes", "x_out", "bstats", "stream",
        "opts"]
    # the reference citations the header uses elsewhere
    for name, cite in (("vc2_gather_rows_grid_chunks", "vidcom2.py:89-91, :93-96, :105-115"),
                       ("vc2_select_chunks_x", "vidcom2.py:70-78"), ("vc2_pool_stats_blocks", "llava_arch.py:171-190")):
        comment = src[:src.index("int " + name)].rsplit("/*", 1)[1]
        assert cite in comment, (name, cite)


def test_options_are_keyword_only_behind_the_existing_arguments():
    for fn in (vc.compress_chunks, vc.ChunkedCompressor.__init__):
        p = inspect.signature(fn).parameters
        assert tuple(p)[-len(OPTIONS):] == OPTIONS, fn
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in OPTIONS)
        assert [p[n].default for n in OPTIONS] == ["linear", 0, None, None, False]
    p = inspect.signature(vc.ChunkedCompressor.add_pooled).parameters
    assert tuple(p) == ("self", "image_feature", "height", "width", "mode") and p["mode"].default == "average"
    assert "Not offered here: `grid_vid`" not in chunked.__doc__ and "img_feat" in chunked.__doc__.split("Not offered")[1]


def _host(n=1024):
    """A non-null pointer that is never dereferenced: every call below is refused on its arguments."""
    return ctypes.cast(ctypes.create_string_buffer(n), ctypes.c_void_p)


def test_c_argument_errors_come_before_any_device_access():
    L = _ffi.lib()
    p = _host()
    table = (ctypes.c_void_p * 2)(p.value, p.value)

    def gather(rows=(8, 4), n_chunks=2, h=2, newline=p, tail=None, tail_rows=0, idx=p, dst=p, dtype=1, tab=table):
        crow = (ctypes.c_int64 * len(rows))(*rows)
        return L.vc2_gather_rows_grid_chunks(tab, crow, n_chunks, h, 8, dtype, idx, None, 4, newline, tail, tail_rows, dst, 4,
                                             None, None)
    assert gather(h=-1) == ERR_ARG
    assert gather(newline=None) == ERR_ARG and "newline" in _ffi.last_error()
    assert gather(rows=(8, 6)) == ERR_ARG and "whole frames" in _ffi.last_error()
    assert gather(tail_rows=-1) == ERR_ARG
    assert gather(tail_rows=1) == ERR_ARG and "tail" in _ffi.last_error()
    assert gather(h=0, newline=None, tail_rows=2) == ERR_ARG
    # ... and vc2_gather_rows_chunks' own checks and codes
    assert gather(n_chunks=0) == ERR_UNSUPPORTED and gather(n_chunks=65) == ERR_UNSUPPORTED
    assert gather(rows=(8, 0)) == ERR_ARG and gather(idx=None) == ERR_ARG and gather(dst=None) == ERR_ARG
    assert gather(dtype=3) == ERR_ARG and gather(tab=None) == ERR_ARG
    assert gather(tab=(ctypes.c_void_p * 2)(p.value, None)) == ERR_ARG

    def select_x(map_mode, grid_h, N, newline, out_rows=p, tail=None, tail_rows=0):
        crow = (ctypes.c_int64 * 2)(N, N)
        return L.vc2_select_chunks_x(p, p, 2, N, 8, 0.25, 1, p, 1 << 20, p, 1 << 30, 1, p, p, 16, p, table, crow, 2, out_rows,
                                     None, None, None, map_mode, grid_h, newline, tail, tail_rows)
    assert select_x(_ffi.MAP_GRID_VID, 3, 10, p) == ERR_ARG and "grid_h" in _ffi.last_error()
    assert select_x(_ffi.MAP_GRID_VID, 0, 9, p) == ERR_ARG
    assert select_x(_ffi.MAP_LINEAR, 0, 9, p) == ERR_ARG and "grid_vid" in _ffi.last_error()      # a newline, no grid
    assert select_x(_ffi.MAP_GRID_VID, 3, 9, None) == ERR_ARG and "newline" in _ffi.last_error()  # rows, no newline
    assert select_x(_ffi.MAP_LOCAL, 0, 9, None) == ERR_ARG
    assert select_x(_ffi.MAP_LINEAR, 0, 9, None, tail_rows=1) == ERR_ARG
    assert select_x(_ffi.MAP_LINEAR, 0, 9, None, tail=p, tail_rows=-1) == ERR_ARG

    def pool(xin=p, H=6, W=6, D=64, mode=1, bf=1, out=p, bstats=p, dtype=1):
        return L.vc2_pool_stats_blocks(xin, 3, H, W, D, dtype, mode, 8, bf, p, 0, out, bstats, None, None)
    assert pool(xin=None) == ERR_ARG and pool(out=None) == ERR_ARG and pool(bstats=None) == ERR_ARG
    assert pool(mode=0) == ERR_ARG and pool(H=1) == ERR_ARG                      # vc2_pool_stats' own
    assert pool(mode=3, D=72) == ERR_UNSUPPORTED and pool(mode=3, H=130, W=130) == ERR_UNSUPPORTED
    assert pool(bf=0) == ERR_ARG and pool(bf=9) == ERR_ARG                       # vc2_chan_stats_o's own
    assert pool() == -5                                                          # VC2_ERR_WORKSPACE: a 0-byte workspace


# ---- 2. the injected-stage route: the definition -------------------------------------------------------------------------

class _ScoringStages(RaggedOracleStages):
    """The oracle-backed CPU stages, leaving their [F_c, N] scores in .v / .f as the driver's want_scores asks."""

    def phase2(self, x, csum_all, R_total):
        self.v, self.f, _ = O.gaussian_scores_sharded(x, self.chan_idx, self.N, csum_all, R_total)
        s, self.total = O.fuse(self.v, self.f)
        return s.float()


class _Factory:
    def __init__(self):
        self.calls = 0

    def __call__(self, F, N, D, dtype, base, frames, rank):
        self.calls += 1
        return _ScoringStages(F, N, D, dtype, base)


def _chunks(x, frames, N):
    out, f0 = [], 0
    for f in frames:
        out.append(x[f0 * N: (f0 + f) * N].clone())
        f0 += f
    return out


def _oracle_grid(x, ref, N, h, newline):
    """The oracle on the concatenation followed by the reference's _map_grid_vid (vidcom2.py:105-115) and the stream
    add_token_per_grid builds."""
    F = x.shape[0] // N
    loc = ref["global_idx"] - torch.repeat_interleave(torch.arange(F) * N, ref["ks"].clamp(max=N))
    gidx = O.map_grid_vid(list(torch.split(loc, ref["ks"].clamp(max=N).tolist())), h)
    stream = torch.cat([x.view(F, h, h, -1), newline.view(1, 1, 1, -1).expand(F, h, 1, -1)], dim=2).reshape(F * h * (h + 1), -1)
    return gidx, stream


def test_grid_and_newline_with_oracle_stages_equal_the_oracle_and_map_grid_vid():
    F, N, h, D, frames = 8, 9, 3, 64, (3, 2, 3)
    x = synth.make(F, N, D, torch.bfloat16, 3, "drift")
    nl = torch.randn(D, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    ref = O.compress_indices(x, N, 0.25)
    gidx, stream = _oracle_grid(x, ref, N, h, nl)
    fac = _Factory()
    res = vc.compress_chunks(_chunks(x, frames, N), N, 0.25, stages_factory=fac, mapper="grid_vid", grid_h=h, newline=nl,
                             want_scores=True)
    assert fac.calls == len(frames)
    assert res.ks.tolist() == ref["ks"].tolist()
    assert res.K == gidx.numel() == int(ref["global_idx"].numel()) + F * h          # K counts the newline rows
    assert torch.equal(res.global_idx, gidx) and torch.equal(res.rows, stream[gidx])
    assert int((res.global_idx % (h + 1) == h).sum()) == F * h
    assert tuple(res.v_score.shape) == (F, N) and res.v_score.dtype == torch.bfloat16
    assert torch.equal(res.v_score, ref["v"]) and torch.equal(res.f_score, ref["f"])
    # a [1, D] newline, no gather: indices are still mapped
    res = vc.compress_chunks(_chunks(x, frames, N), N, 0.25, gather=False, stages_factory=fac, mapper="grid_vid", grid_h=h,
                             newline=nl[None])
    assert res.rows is None and torch.equal(res.global_idx, gidx) and res.v_score is None


@pytest.mark.parametrize("m", [1, 2])
def test_tail_rows_with_oracle_stages_follow_the_kept_rows(m):
    F, N, D, frames = 8, 49, 64, (3, 2, 3)
    x = synth.make(F, N, D, torch.bfloat16, 3, "drift")
    tail = torch.randn(m, D, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    ref = O.compress_indices(x, N, 0.25)
    want = torch.cat([x[ref["global_idx"]], tail])
    fac = _Factory()
    res = vc.compress_chunks(_chunks(x, frames, N), N, 0.25, stages_factory=fac, tail=tail if m > 1 else tail[0],
                             want_scores=True)
    assert res.K == int(ref["global_idx"].numel()) and tuple(res.rows.shape) == (res.K + m, D)
    assert torch.equal(res.global_idx, ref["global_idx"]) and torch.equal(res.rows, want)
    assert res.ks.tolist() == ref["ks"].tolist()
    assert torch.equal(res.v_score, ref["v"]) and torch.equal(res.f_score, ref["f"])
    # the compressor object: another tail of the same shape for the next video, none of another
    cc = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, "cpu", 0.25, stages_factory=fac, tail=tail)
    assert torch.equal(cc(_chunks(x, frames, N)).rows, want)
    assert torch.equal(cc(_chunks(x, frames, N), tail=tail + 1).rows, torch.cat([x[ref["global_idx"]], tail + 1]))
    with pytest.raises(RuntimeError, match="tail must be"):
        cc(_chunks(x, frames, N), tail=torch.zeros(m + 1, D, dtype=torch.bfloat16))


# ---- 3. the argument errors, with nothing built or enqueued --------------------------------------------------------------

def test_argument_errors_mirror_compress_and_build_nothing():
    fac = _Factory()
    N, h, D = 9, 3, 8
    a = torch.zeros(2 * N, D, dtype=torch.bfloat16)
    nl = torch.zeros(D, dtype=torch.bfloat16)

    def both(err, match, **kw):
        with pytest.raises(err, match=match):
            vc.compress_chunks([a, a], N, stages_factory=fac, **kw)
        with pytest.raises(err, match=match):
            vc.ChunkedCompressor([2, 2], N, D, torch.bfloat16, "cpu", stages_factory=fac, **kw)
        with pytest.raises(err, match=match):                                # the device route: refused before the device
            vc.compress_chunks([a, a], N, **kw)
    both(ValueError, "newline is the grid_vid mapper's newline vector", newline=nl)
    both(ValueError, "newline is the grid_vid mapper's newline vector", mapper="linear", grid_h=h, newline=nl)
    both(ValueError, "img_feat required for grid mapping", mapper="grid_vid", grid_h=h)
    both(ValueError, "unknown mapper", mapper="grid")
    both(RuntimeError, r"grid_vid mapping needs N == grid_h\^2", mapper="grid_vid", grid_h=4, newline=nl)
    both(RuntimeError, r"grid_vid mapping needs N == grid_h\^2", mapper="grid_vid", newline=nl)
    for bad in (torch.zeros(D), torch.zeros(D + 1, dtype=torch.bfloat16), torch.zeros(2, D, dtype=torch.bfloat16), "nl"):
        both(RuntimeError, "newline must be a", mapper="grid_vid", grid_h=h, newline=bad)
    for bad in (torch.zeros(1, D), torch.zeros(1, D + 1, dtype=torch.bfloat16), torch.zeros(1, 1, D, dtype=torch.bfloat16), 3):
        both(RuntimeError, "tail must be", tail=bad)
    assert fac.calls == 0
    with pytest.raises(TypeError):                                            # keyword-only
        vc.compress_chunks([a, a], N, 0.25, True, None, None, fac, "grid_vid")
    # what compress words the same way (its own checks come before its device check)
    x = torch.zeros(2 * N, D)
    with pytest.raises(ValueError, match="newline is the grid_vid mapper's newline vector"):
        vc.compress(x, N, newline=torch.zeros(D))
    with pytest.raises(ValueError, match="img_feat required for grid mapping"):
        vc.map_features([torch.arange(2)] * 2, x, None, dict(mapper="grid_vid", grid=h))


def test_add_pooled_validates_like_pool_stats_and_needs_the_hip_stages():
    fac = _Factory()
    cc = vc.ChunkedCompressor([2, 2], 9, 64, torch.bfloat16, "cpu", stages_factory=fac)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # fused.pool_stats' first check
        cc.add_pooled(torch.zeros(2, 36, 64, dtype=torch.bfloat16), 6, 6)
    assert cc._chunks == [] and cc._pending is None


def test_one_chunk_delegates_to_compress_with_the_options(monkeypatch):
    seen = {}

    def fake(x, tpf, base_scale=0.25, **kw):
        seen.update(kw)
        return "delegated"
    monkeypatch.setattr(chunked._vc, "compress", fake)
    x, nl = torch.zeros(2 * 9, 8, dtype=torch.bfloat16), torch.zeros(8, dtype=torch.bfloat16)
    assert vc.compress_chunks([x], 9, mapper="grid_vid", grid_h=3, newline=nl, want_scores=True) == "delegated"
    assert seen["mapper"] == "grid_vid" and seen["grid_h"] == 3 and seen["newline"] is nl and seen["want_scores"] is True
    assert seen["tail"] is None and seen["gather"] is True

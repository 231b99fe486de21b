"""A video held as frame chunks (vidcom2_amd/chunked.py) on the GPU: the chunk gather through the C ABI, the chunked pass
against the unsharded pass and the oracle (bit for bit, no tolerances), its launches, its memory, reuse and autograd.
Every pass test first asserts that the unsharded pass equals its reference on the same input, so that a failure points at
the chunked path."""
import ctypes
import gc
import warnings

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, chunked, synth
from vidcom2_amd._ffi import DTYPE_CODE, lib, ptr, stream_ptr

from _ragged_shards import DTYPES
from _sharded_params import params_of
from _stage_chain import digest
import _score_dtype as SD
from conftest import load_json, make_input
from test_ragged_shards import _Spy, _reference

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _split(xd, frames, N):
    out, f0 = [], 0
    for f in frames:
        out.append(xd[f0 * N: (f0 + f) * N].clone())
        f0 += f
    return out


@pytest.fixture
def _modes():
    _ffi.set_mode("torch")
    O.set_mode("torch")
    yield
    _ffi.set_mode("torch")
    O.set_mode("exact")


# ---- 1. the gather alone, through the C ABI -----------------------------------------------------------------------------

SENTINEL = 77.0


def _make_chunks(rows, D, dtype, misaligned=None):
    """Chunks of distinct values; chunk `misaligned` is a view at element offset 1 of a larger buffer."""
    g = torch.Generator().manual_seed(5)
    out = []
    for c, r in enumerate(rows):
        vals = torch.randn(r, D, generator=g).to(dtype).to(dev())
        if c == misaligned:
            big = torch.zeros(r * D + 8, dtype=dtype, device=dev())
            view = big[1: 1 + r * D].view(r, D)
            view.copy_(vals)
            assert view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
            vals = view
        out.append(vals)
    return out


def _gather(chunks, idx, n_dev, n_max, dst, dst_rows, n_chunks=None, rows=None):
    """vc2_gather_rows_chunks on the current stream; returns (return code, status word)."""
    n_chunks = len(chunks) if n_chunks is None else n_chunks
    table = (ctypes.c_void_p * len(chunks))(*[c.data_ptr() for c in chunks])
    crow = (ctypes.c_int64 * len(chunks))(*(rows if rows is not None else [c.shape[0] for c in chunks]))
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    D, dtype = chunks[0].shape[1], chunks[0].dtype
    rc = lib().vc2_gather_rows_chunks(table, crow, n_chunks, D, DTYPE_CODE[dtype], ptr(idx), ptr(n_dev), n_max, ptr(dst),
                                      dst_rows, ptr(status), stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, int(status.item())


def _edge_indices(rows):
    """The first and the last row of every chunk, then every row once more, in a scrambled order."""
    starts = chunked.chunk_starts(rows)
    edge = [r for c in range(len(rows)) for r in (starts[c], starts[c + 1] - 1)]
    g = torch.Generator().manual_seed(9)
    return torch.tensor(edge + torch.randperm(starts[-1], generator=g).tolist(), dtype=torch.int64)


@pytest.mark.parametrize("rows", [(3, 1, 7), (1,) * 64], ids=["3+1+7", "64x1"])
@pytest.mark.parametrize("D,dn,misaligned", [(64, "bf16", None), (100, "f16", None), (3, "f32", None), (64, "bf16", 1),
                                             (100, "f16", 1)],
                         ids=["64-bf16", "100-f16", "3-f32", "64-bf16-chunk1-at-offset-1", "100-f16-chunk1-at-offset-1"])
def test_gather_rows_chunks_equals_cat_index(rows, D, dn, misaligned):
    """dst[j] = cat(chunks)[idx[j]] for j < n (n on the device, below n_max): row bytes a multiple of 16 and not, a chunk
    whose base is aligned to its element size only (the byte path), the first and last row of every chunk; the rows behind
    n and a guard region behind dst keep their fill."""
    dtype = DTYPES[dn]
    chunks = _make_chunks(rows, D, dtype, misaligned)
    want = torch.cat(chunks)
    idx = _edge_indices(rows).to(dev())
    n_max, n, guard = idx.numel(), idx.numel() - 3, 5
    dst = torch.full((n_max + guard, D), SENTINEL, dtype=dtype, device=dev())
    rc, status = _gather(chunks, idx, torch.tensor([n], device=dev()), n_max, dst, n_max)
    assert (rc, status) == (0, 0), _ffi.last_error()
    assert torch.equal(dst[:n], want[idx[:n]])
    assert bool((dst[n:] == SENTINEL).all())
    # n_dev NULL: n_max rows
    dst.fill_(SENTINEL)
    rc, status = _gather(chunks, idx, None, n_max, dst, n_max)
    assert (rc, status) == (0, 0)
    assert torch.equal(dst[:n_max], want[idx]) and bool((dst[n_max:] == SENTINEL).all())


def test_gather_rows_chunks_reports_rows_it_cannot_place():
    rows, D, dtype = (3, 1, 7), 64, torch.bfloat16
    chunks = _make_chunks(rows, D, dtype)
    want = torch.cat(chunks)
    idx = _edge_indices(rows).to(dev())
    n = idx.numel()
    # a destination smaller than n: bit 2, nothing behind dst_rows is written
    small = 4
    dst = torch.full((n + 5, D), SENTINEL, dtype=dtype, device=dev())
    rc, status = _gather(chunks, idx, torch.tensor([n], device=dev()), n, dst, small)
    assert rc == 0 and status & 2
    assert torch.equal(dst[:small], want[idx[:small]]) and bool((dst[small:] == SENTINEL).all())
    # one index equal to sum(chunk_rows), one negative: bit 2, those rows untouched, all others correct
    bad = idx.clone()
    bad[2], bad[5] = sum(rows), -1
    dst.fill_(SENTINEL)
    rc, status = _gather(chunks, bad, torch.tensor([n], device=dev()), n, dst, n)
    assert rc == 0 and status & 2
    ok = torch.ones(n, dtype=torch.bool, device=dev())
    ok[2] = ok[5] = False
    assert torch.equal(dst[:n][ok], want[idx[ok]])
    assert bool((dst[:n][~ok] == SENTINEL).all()) and bool((dst[n:] == SENTINEL).all())


def test_gather_rows_chunks_refuses_bad_tables_and_enqueues_nothing():
    D, dtype = 64, torch.bfloat16
    chunks = _make_chunks((1,) * 65, D, dtype)
    idx = torch.arange(8, dtype=torch.int64, device=dev())
    dst = torch.full((8, D), SENTINEL, dtype=dtype, device=dev())
    rc, status = _gather(chunks, idx, None, 8, dst, 8)
    assert rc == -3 and status == 0 and "65 chunks" in _ffi.last_error()          # VC2_ERR_UNSUPPORTED
    assert _gather(chunks[:3], idx, None, 8, dst, 8, n_chunks=0)[0] == -3
    assert _gather(chunks[:3], idx, None, 8, dst, 8, rows=[1, 0, 1])[0] == -1      # VC2_ERR_ARG
    assert _gather(chunks[:3], None, None, 8, dst, 8)[0] == -1
    assert _gather(chunks[:3], idx, None, 8, None, 8)[0] == -1
    table = (ctypes.c_void_p * 2)(chunks[0].data_ptr(), None)
    crow = (ctypes.c_int64 * 2)(1, 1)
    assert lib().vc2_gather_rows_chunks(table, crow, 2, D, 1, ptr(idx), None, 8, ptr(dst), 8, None, stream_ptr(dev())) == -1
    assert lib().vc2_gather_rows_chunks(None, crow, 2, D, 1, ptr(idx), None, 8, ptr(dst), 8, None, stream_ptr(dev())) == -1
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())


# ---- 2. - 4. the chunked pass against the unsharded pass and the oracle ---------------------------------------------------

def _assert_equals_whole(res, x, ref, rows, gidx):
    assert res.ks.cpu().tolist() == ref["ks"].tolist()
    assert res.K == int(ref["global_idx"].numel()) == int(res.global_idx.numel())
    assert torch.equal(res.global_idx, gidx) and torch.equal(res.global_idx.cpu(), ref["global_idx"])
    assert torch.equal(res.rows, rows)
    assert torch.equal(res.rows.cpu(), x[ref["global_idx"]])


@pytest.mark.parametrize("dn", ["bf16", "f16"])
@pytest.mark.parametrize("frames", [(16, 32), (32, 16), (16, 16, 16)], ids=lambda f: "+".join(map(str, f)))
def test_chunks_of_multiples_of_16_frames_equal_the_unsharded_pass(dn, frames):
    """48 x 49 x 256, seed 1, base 0.25, warnings as errors: budgets, kept indices, K and rows are compress(cat)'s and the
    oracle's."""
    F, N, D = 48, 49, 256
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 1, 0.25, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])                             # the unsharded pass itself
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, N), N, 0.25)
    _assert_equals_whole(res, x, ref, rows, gidx)


@pytest.mark.parametrize("case", [(16, 169, 512, "f16", 0.15, (7, 2, 7)), (16, 196, 1024, "f32", 0.25, (5, 11)),
                                  (24, 196, 3584, "bf16", 0.25, (5, 19))],
                         ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[5])))
def test_unequal_chunks_equal_the_unsharded_pass(case):
    """The cases test_unequal_shards_equal_the_unsharded_pass proves on these kernels, same inputs (seed 1), default mode,
    warnings as errors; the whole-video scores are the unsharded pass's too (16-bit)."""
    F, N, D, dn, base, frames = case
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 1, base, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    cc = vc.ChunkedCompressor(frames, N, D, DTYPES[dn], dev(), base)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = cc(_split(xd, frames, N))
    _assert_equals_whole(res, x, ref, rows, gidx)
    assert cc.vc_fragile == 0
    if dn != "f32":
        assert torch.equal(cc._total, total)
    assert all(s.mask.data_ptr() == cc.stages[0].mask.data_ptr() for s in cc.stages)     # one channel set, shared


@pytest.mark.parametrize("case", [(8, 49, 64, "bf16", (3, 2, 3)), (12, 5, 128, "f16", (5, 1, 1, 5)),
                                  (6, 49, 64, "bf16", (2, 1, 3), 8)],
                         ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[4])) + ("-cap8" if len(c) > 5 else ""))
def test_replay_rounds_across_chunks(case):
    """Library mode 2 flags every video-centre column, so all of them go through the ragged exchange 2b -- in rounds, more
    than one with vc_cap = 8 -- on the shared record buffer: kept indices are the oracle's, the whole-video scores the
    unsharded pass's in the same mode, no fragile column remains."""
    F, N, D, dn, frames = case[:5]
    cap = case[5] if len(case) > 5 else D // 2
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 2, 0.25, 2)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    log = []
    try:
        assert _ffi.lib().vc2_set_mode(2) == 0
        cc = vc.ChunkedCompressor(frames, N, D, DTYPES[dn], dev(), 0.25, vc_cap=cap)
        for s in cc.stages:
            s._L = _Spy(s._L, log)
        res = cc(_split(xd, frames, N))
    finally:
        _ffi.set_mode("torch")
    called = [n for n, _ in log]
    assert "vc2_video_centre_blocks_ragged" in called and "vc2_video_centre_finish_round_ragged" in called
    if len(case) > 5:
        assert "vc2_video_centre_blocks_round_ragged" in called
    assert called.count("vc2_video_centre_flagged") == 1                          # one host read for all chunks
    assert cc.vc_fragile == 0
    assert torch.equal(cc._total, total)
    assert torch.equal(res.global_idx.cpu(), ref["global_idx"]) and res.ks.cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(res.rows, rows)


# ---- 5. params and score_dtype ---------------------------------------------------------------------------------------------

def test_chunks_with_params_equal_the_reference(_modes):
    """("rt", 12, 196, 1024, bf16) of tests/golden/pass_params_cases.json in chunks (5, 7): the recorded reference results and
    compress(cat, params=...)."""
    name, F, N, D, dn, frames = "rt", 12, 196, 1024, "bf16", (5, 7)
    (c,) = [c for c in load_json("pass_params_cases.json")["cases"]
            if (c["name"], c["F"], c["N"], c["D"], c["dtype"]) == (name, F, N, D, dn)]
    x = make_input(F, N, D, dn, c["seed"], c["dist"])
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    xd = x.to(dev())
    p = params_of(c)
    whole = vc.compress(xd, N, c["base"], params=p)
    assert whole.ks.cpu().tolist() == c["ks"] and whole.K == c["K"]
    assert digest(whole.global_idx) == c["keep_sha256"] and digest(whole.rows) == c["rows_sha256"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, N), N, c["base"], params=p)
    assert res.ks.cpu().tolist() == c["ks"] and res.K == c["K"]
    assert digest(res.global_idx) == c["keep_sha256"] and digest(res.rows) == c["rows_sha256"]
    assert torch.equal(res.ks, whole.ks) and torch.equal(res.global_idx, whole.global_idx)
    assert torch.equal(res.rows, whole.rows)


def test_chunks_scored_in_fp32_equal_the_reference(_modes):
    """16 x 169 x 512 bf16 (drift, seed 0) of tests/golden/score_dtype_cases.json in chunks (5, 11),
    score_dtype=torch.float32: the recorded reference results and compress(cat, score_dtype=torch.float32); rows in bf16."""
    key, frames = (16, 169, 512, "bf16", "drift", 0, None), (5, 11)
    (c,) = [c for c in SD.load() if (c["F"], c["N"], c["D"], c["dtype"], c["dist"], c["seed"], c["ratio"], c["mapper"],
                                      c["base"]) == key + ("linear", 0.25)]
    x = SD.make_input(c)
    assert synth.sha256_tensor(x) == c["x_sha256"], "synthetic generator is not bit-portable"
    xd = x.to(dev())
    whole = vc.compress(xd, c["N"], c["base"], score_dtype=torch.float32)
    assert whole.ks.cpu().tolist() == c["ks"] and whole.global_idx.cpu().tolist() == c["global_idx"] and whole.K == c["K"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, c["N"]), c["N"], c["base"], score_dtype=torch.float32)
    assert res.ks.cpu().tolist() == c["ks"] and res.global_idx.cpu().tolist() == c["global_idx"] and res.K == c["K"]
    assert torch.equal(res.ks, whole.ks) and torch.equal(res.global_idx, whole.global_idx)
    assert res.rows.dtype == torch.bfloat16 and torch.equal(res.rows, whole.rows)
    assert torch.equal(res.rows.cpu(), x[res.global_idx.cpu()])


# ---- 6. one sync, one selection ------------------------------------------------------------------------------------------

def test_one_selection_one_channel_selection_one_host_read(monkeypatch):
    F, N, D, frames = 8, 49, 64, (3, 2, 3)
    x, xd, ref, total, rows, gidx = _reference(F, N, D, "bf16", 2, 0.25, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    cc = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, dev(), 0.25)
    log = []
    cc._L = _Spy(cc._L, log)
    for s in cc.stages:
        s._L = _Spy(s._L, log)
    reads = []
    for name in ("tolist", "item", "cpu"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    f0 = 0
    for c, f in enumerate(frames):
        chunk = xd[f0 * N: (f0 + f) * N].clone()                      # (the next chunk does not exist before this add returns)
        f0 += f
        del reads[:]
        cc.add(chunk)
        names = [n for n, _ in log]
        assert names.count("vc2_chan_stats") + names.count("vc2_chan_stats_o") == c + 1
        if c + 1 < len(frames):
            assert set(names) <= {"vc2_chan_stats", "vc2_chan_stats_o"}, names
        assert reads == []                                            # add never reads the device
    res = cc.finish()
    assert reads == ["tolist"]                                        # the pass's single host sync
    monkeypatch.undo()
    names = [n for n, _ in log]
    assert names.count("vc2_select_chunks") + names.count("vc2_select_chunks_o") == 1
    assert not any(n.startswith("vc2_select_sharded") for n in names)
    assert names.count("vc2_chan_select") == 1 and names.count("vc2_chan_var_from_stats") == 1
    assert names.count("vc2_scores_phase1") == len(frames)
    assert torch.equal(res.global_idx.cpu(), ref["global_idx"]) and torch.equal(res.rows, rows)


# ---- 7. memory -----------------------------------------------------------------------------------------------------------

MEM_SHAPE = (32, 1024, 512, "bf16", (16, 16))


def _chunked_bytes_on_the_host(F, N, D, dtype, frames, base=0.25):
    """Workspaces and outputs of the chunked pass, from the host: every chunk's stage workspace, the whole-video
    exchange buffers, the selection scratch and the outputs (kept rows, indices, budgets)."""
    es = torch.empty(0, dtype=dtype).element_size()
    ws = sum(_ffi.workspace_bytes(f, N, D, dtype) for f in frames)
    C, W = D // 2, len(frames)
    bf = chunked.stat_block_frames(frames)
    shared = (F // bf) * 2 * D * 8 + W * 2 * max((f + 15) // 16 for f in frames) * C * 8 \
        + W * 64 * (2 * 256 + 1 + max(frames) * N // 16) * 4 + F * 4 + F * N * 4 + D * 17
    n = ctypes.c_size_t(0)
    assert lib().vc2_select_chunks_ws_bytes(F, ctypes.byref(n)) == 0
    cap = min(F * N, int(lib().vc2_kept_capacity(F, N, base)))
    outputs = cap * D * es + cap * 8 + F * 8 + 32
    per_stage = sum(min(f * N, int(lib().vc2_kept_capacity(f + 1, N, base))) * 8 + f * 8 + 32 for f in frames)
    return ws + shared + int(n.value) + outputs + per_stage


def _peak_above(fn):
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, out


def test_chunked_pass_allocates_less_than_the_video():
    """32 x 1024 x 512 bf16 in chunks (16, 16), a video of 33.6 MB: of the shapes tried in ascending order below the first
    at which the chunked pass's workspaces plus outputs, computed on the host, stay below half of the video's bytes (0.48 of
    them; a search over F in 8..128, N in 196..4096, D in 64..2048 finds no smaller video that does).  With the chunks
    resident, compress_chunks allocates less than the video's bytes at its peak; torch.cat + compress at least the video."""
    tried = [(8, 49, 64, "bf16", (4, 4)), (16, 196, 256, "bf16", (8, 8)), (32, 196, 1024, "bf16", (16, 16)),
             (32, 729, 512, "bf16", (16, 16)), MEM_SHAPE]
    first = None
    for F, N, D, dn, frames in tried:
        video = F * N * D * 2
        est = _chunked_bytes_on_the_host(F, N, D, DTYPES[dn], frames)
        print((F, N, D, dn, frames), "video", video, "workspaces + outputs", est)
        if first is None and est < video / 2:
            first = (F, N, D, dn, frames)
    assert first == MEM_SHAPE
    F, N, D, dn, frames = MEM_SHAPE
    video = F * N * D * 2
    xd = synth.make(F, N, D, DTYPES[dn], 1, "drift").to(dev())
    chunks = _split(xd, frames, N)
    whole = vc.compress(xd, N, 0.25)
    del xd
    vc.vidcom2.clear_plan_cache()
    chunked.clear_chunk_cache()
    peak_a, res = _peak_above(lambda: vc.compress_chunks(chunks, N, 0.25))
    chunked.clear_chunk_cache()
    peak_b, res_b = _peak_above(lambda: vc.compress(torch.cat(chunks), N, 0.25))
    print("video", video, "peak compress_chunks", peak_a, "peak cat + compress", peak_b)
    assert torch.equal(res.global_idx, whole.global_idx) and torch.equal(res.rows, whole.rows)
    assert torch.equal(res_b.global_idx, whole.global_idx)
    assert peak_a < video
    assert peak_b >= video


# ---- 8. reuse ------------------------------------------------------------------------------------------------------------

def test_one_compressor_two_videos():
    F, N, D, frames = 16, 49, 64, (5, 11)
    cc = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, dev(), 0.25)
    got, want = [], []
    for seed in (1, 2, 1):
        xd = synth.make(F, N, D, torch.bfloat16, seed, "drift").to(dev())
        want.append(vc.compress(xd, N, 0.25))
        got.append(cc(_split(xd, frames, N)))
    assert not torch.equal(want[0].global_idx, want[1].global_idx)    # two different videos
    for g, w in zip(got, want):                                       # (every result still holds its own video's values)
        assert g.K == w.K and torch.equal(g.ks, w.ks) and torch.equal(g.global_idx, w.global_idx)
        assert torch.equal(g.rows, w.rows)


# ---- 9. autograd ----------------------------------------------------------------------------------------------------------

def test_rows_carry_gradients_to_every_chunk():
    F, N, D, frames = 16, 49, 64, (5, 11)
    x = synth.make(F, N, D, torch.float32, 1, "drift")
    O.set_mode("torch")
    try:
        ref = O.compress_indices(x, N, 0.25)
    finally:
        O.set_mode("exact")
    xd = x.to(dev())
    assert torch.equal(vc.compress(xd, N, 0.25).global_idx.cpu(), ref["global_idx"])
    chunks = [c.requires_grad_() for c in _split(xd, frames, N)]
    res = vc.compress_chunks(chunks, N, 0.25)
    assert res.rows.requires_grad and torch.equal(res.global_idx.cpu(), ref["global_idx"])
    g = torch.randn(res.rows.shape, generator=torch.Generator().manual_seed(3)).to(dev())
    got = torch.autograd.grad(res.rows, chunks, g)
    leaves = [c.detach().clone().requires_grad_() for c in chunks]
    want = torch.autograd.grad(torch.cat(leaves)[res.global_idx], leaves, g)
    assert torch.equal(res.rows.detach(), torch.cat(leaves)[res.global_idx].detach())
    for a, b, c in zip(got, want, chunks):
        assert a.shape == c.shape and torch.equal(a, b)
    assert all(int((a != 0).any(1).sum()) > 0 for a in got)           # each chunk kept rows; dropped tokens get zero rows
    # only the second chunk requires grad
    chunks2 = [chunks[0].detach(), chunks[1]]
    res2 = vc.compress_chunks(chunks2, N, 0.25)
    (g1,) = torch.autograd.grad(res2.rows, [chunks2[1]], g)
    assert torch.equal(g1, want[1])
    with torch.no_grad():
        res3 = vc.compress_chunks(chunks, N, 0.25)
    assert res3.rows.grad_fn is None and not res3.rows.requires_grad
    assert torch.equal(res3.rows, res.rows.detach())

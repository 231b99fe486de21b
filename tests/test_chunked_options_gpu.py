"""The options `compress` takes from the LLaVA hooks, in the chunked pass, on the GPU: the gather that understands chunks,
grid slots, the newline vector and tail rows at once (vc2_gather_rows_grid_chunks, through the C ABI, against torch indexing
on the stream torch builds from torch.cat(chunks) and the newline); the whole pass with each option against
`compress(torch.cat(chunks), ...)` with the same options and against the oracle (torch.equal; fp32 scores within the 1e-6 of
DESIGN.md section 3); pooled chunks (`add_pooled`) against `fused.pool_stats` + `add`; the gradients against torch's."""
import ctypes
import warnings

import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import _ffi, chunked, fused, synth
from vidcom2_amd._ffi import DTYPE_CODE, lib, ptr, stream_ptr

from _ragged_shards import DTYPES
from _sharded_params import params_of
import _score_dtype as SD
from conftest import load_json, make_input
from test_ragged_shards import _Spy, _reference

pytestmark = pytest.mark.gpu

SENTINEL = 77.0
H = 2                                      # the gather tests' grid: frames of 2 x 2 tokens, 2 newline slots each


def dev():
    return torch.device("cuda:0")


def _split(xd, frames, N):
    out, f0 = [], 0
    for f in frames:
        out.append(xd[f0 * N: (f0 + f) * N].clone())
        f0 += f
    return out


def _at_offset_1(vals):
    """`vals` as a contiguous view at element offset 1 of a larger buffer: aligned to its element size only."""
    big = torch.zeros(vals.numel() + 8, dtype=vals.dtype, device=vals.device)
    view = big[1: 1 + vals.numel()].view(vals.shape)
    view.copy_(vals)
    assert view.data_ptr() % 16 == view.element_size() and view.is_contiguous()
    return view


def _make(frames, D, dtype, misaligned=None, h=H):
    """Chunks of frames[c] * h * h rows of distinct values, a newline vector and two tail rows; chunk `misaligned` and
    -- then -- the newline sit at element offset 1 of their buffers."""
    g = torch.Generator().manual_seed(5)
    chunks = [torch.randn(f * h * h, D, generator=g).to(dtype).to(dev()) for f in frames]
    nl = torch.randn(D, generator=g).to(dtype).to(dev())
    tail = torch.randn(2, D, generator=g).to(dtype).to(dev())
    if misaligned is not None:
        chunks[misaligned] = _at_offset_1(chunks[misaligned])
        nl = _at_offset_1(nl)
    return chunks, nl, tail


def _stream(chunks, nl, h):
    """What add_token_per_grid builds from the concatenation and the newline vector: [F * h * (h + 1), D]."""
    x = torch.cat(chunks)
    F, D = x.shape[0] // (h * h), x.shape[1]
    return torch.cat([x.view(F, h, h, D), nl.view(1, 1, 1, D).expand(F, h, 1, D)], dim=2).reshape(F * h * (h + 1), D)


def _gather(chunks, h, idx, n_dev, n_max, nl, tail, tail_rows, dst, dst_rows, n_chunks=None, rows=None, dtype=None):
    """vc2_gather_rows_grid_chunks on the current stream; returns (return code, status word)."""
    n_chunks = len(chunks) if n_chunks is None else n_chunks
    table = (ctypes.c_void_p * len(chunks))(*[c.data_ptr() if c is not None else None for c in chunks])
    crow = (ctypes.c_int64 * len(chunks))(*(rows if rows is not None else [c.shape[0] for c in chunks]))
    status = torch.zeros(1, dtype=torch.int32, device=dev())
    D = dst.shape[1] if dst is not None else 64
    code = DTYPE_CODE[dst.dtype] if dtype is None else dtype
    rc = lib().vc2_gather_rows_grid_chunks(table, crow, n_chunks, h, D, code, ptr(idx), ptr(n_dev), n_max, ptr(nl), ptr(tail),
                                           tail_rows, ptr(dst), dst_rows, ptr(status), stream_ptr(dev()))
    torch.cuda.synchronize()
    return rc, int(status.item())


def _edge_slots(frames, h):
    """The first and the last slot of every chunk (the last one is a newline slot) and its last token slot, every newline
    slot of the first and of the last frame, then every slot once more in a scrambled order."""
    w, fw = h + 1, h * (h + 1)
    starts = chunked.chunk_starts([f * fw for f in frames])
    edge = [s for c in range(len(frames)) for s in (starts[c], starts[c + 1] - 1, starts[c + 1] - 2)]
    F = sum(frames)
    edge += [f * fw + r * w + h for f in (0, F - 1) for r in range(h)]
    g = torch.Generator().manual_seed(9)
    return torch.tensor(edge + torch.randperm(starts[-1], generator=g).tolist(), dtype=torch.int64)


# ---- 1. the gather alone, through the C ABI -----------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [(3, 1, 7), (1,) * 64], ids=["3+1+7", "64x1"])
@pytest.mark.parametrize("D,dn,misaligned", [(64, "bf16", None), (100, "f16", None), (3, "f32", None), (64, "bf16", 1),
                                             (100, "f16", 1)],
                         ids=["64-bf16", "100-f16", "3-f32", "64-bf16-chunk1-and-newline-at-offset-1",
                              "100-f16-chunk1-and-newline-at-offset-1"])
def test_gather_equals_index_of_the_torch_built_stream(frames, D, dn, misaligned):
    """dst[j] = stream[idx[j]] for j < n (n on the device, below n_max) at h = 2, followed by 0, 1 and 2 tail rows: the
    table limit of 64 chunks, row bytes a multiple of 16 and not, a chunk and the newline aligned to their element size only
    (copy_row's byte path); what lies behind the last written row, a guard region included, keeps its fill."""
    chunks, nl, tail = _make(frames, D, DTYPES[dn], misaligned)
    want = _stream(chunks, nl, H)
    idx = _edge_slots(frames, H).to(dev())
    n_max, n, guard = idx.numel(), idx.numel() - 3, 5
    dst = torch.full((n_max + 2 + guard, D), SENTINEL, dtype=DTYPES[dn], device=dev())
    for m in (0, 1, 2):
        dst.fill_(SENTINEL)
        rc, status = _gather(chunks, H, idx, torch.tensor([n], device=dev()), n_max, nl, tail if m else None, m, dst, n_max + m)
        assert (rc, status) == (0, 0), _ffi.last_error()
        assert torch.equal(dst[:n], want[idx[:n]]) and torch.equal(dst[n: n + m], tail[:m])
        assert bool((dst[n + m:] == SENTINEL).all())
    dst.fill_(SENTINEL)                                                   # n_dev NULL: n_max rows
    rc, status = _gather(chunks, H, idx, None, n_max, nl, tail, 2, dst, n_max + 2)
    assert (rc, status) == (0, 0)
    assert torch.equal(dst[:n_max], want[idx]) and torch.equal(dst[n_max: n_max + 2], tail)
    assert bool((dst[n_max + 2:] == SENTINEL).all())


@pytest.mark.parametrize("m", [1, 2])
def test_rows_of_the_concatenation_with_tail_rows_equal_the_chunk_gather_plus_the_tail(m):
    """h = 0: idx[] holds rows of the virtual concatenation -- vc2_gather_rows_chunks' result, the tail behind it."""
    frames, D, dtype = (3, 1, 7), 100, torch.float16
    chunks, nl, tail = _make(frames, D, dtype, misaligned=1)
    R = sum(c.shape[0] for c in chunks)
    idx = torch.randperm(R, generator=torch.Generator().manual_seed(3)).to(dev())
    n = R - 2
    plain = torch.full((R, D), SENTINEL, dtype=dtype, device=dev())
    table = (ctypes.c_void_p * len(chunks))(*[c.data_ptr() for c in chunks])
    crow = (ctypes.c_int64 * len(chunks))(*[c.shape[0] for c in chunks])
    n_dev = torch.tensor([n], device=dev())
    assert lib().vc2_gather_rows_chunks(table, crow, len(chunks), D, DTYPE_CODE[dtype], ptr(idx), ptr(n_dev), R, ptr(plain), R,
                                        None, stream_ptr(dev())) == 0
    dst = torch.full((R + m + 3, D), SENTINEL, dtype=dtype, device=dev())
    rc, status = _gather(chunks, 0, idx, n_dev, R, None, tail, m, dst, R + m)
    assert (rc, status) == (0, 0), _ffi.last_error()
    assert torch.equal(dst[:n], plain[:n]) and torch.equal(dst[:n], torch.cat(chunks)[idx[:n]])
    assert torch.equal(dst[n: n + m], tail[:m]) and bool((dst[n + m:] == SENTINEL).all())


def test_gather_reports_what_it_cannot_place_and_touches_nothing_else():
    frames, D, dtype = (3, 1, 7), 64, torch.bfloat16
    chunks, nl, tail = _make(frames, D, dtype)
    want = _stream(chunks, nl, H)
    idx = _edge_slots(frames, H).to(dev())
    n = idx.numel()
    # a destination one row short of n + 2: bit 2, the last tail row is not written, nothing behind dst_rows is
    dst = torch.full((n + 2 + 5, D), SENTINEL, dtype=dtype, device=dev())
    rc, status = _gather(chunks, H, idx, torch.tensor([n], device=dev()), n, nl, tail, 2, dst, n + 1)
    assert rc == 0 and status & 2
    assert torch.equal(dst[:n], want[idx]) and torch.equal(dst[n], tail[0]) and bool((dst[n + 1:] == SENTINEL).all())
    # a slot equal to the slot count, one behind the token rows' count but inside the slot space, a negative one
    space, tokens = want.shape[0], sum(c.shape[0] for c in chunks)
    assert tokens < space
    bad = idx.clone()
    bad[2], bad[5], bad[7] = space, -1, tokens                            # (bad[7] is a valid SLOT: it must be gathered)
    dst.fill_(SENTINEL)
    rc, status = _gather(chunks, H, bad, torch.tensor([n], device=dev()), n, nl, tail, 2, dst, n + 2)
    assert rc == 0 and status & 2
    ok = torch.ones(n, dtype=torch.bool, device=dev())
    ok[2] = ok[5] = False
    assert torch.equal(dst[:n][ok], want[bad[ok]])
    assert bool((dst[:n][~ok] == SENTINEL).all()) and torch.equal(dst[n: n + 2], tail)
    assert bool((dst[n + 2:] == SENTINEL).all())
    # rows of the concatenation (h = 0): an index equal to the row count
    bad = torch.tensor([0, tokens, tokens - 1], device=dev())
    dst.fill_(SENTINEL)
    rc, status = _gather(chunks, 0, bad, None, 3, None, None, 0, dst, 3)
    assert rc == 0 and status & 2
    x = torch.cat(chunks)
    assert torch.equal(dst[0], x[0]) and torch.equal(dst[2], x[-1]) and bool((dst[1] == SENTINEL).all())
    assert bool((dst[3:] == SENTINEL).all())


def test_gather_refuses_bad_tables_and_arguments_and_enqueues_nothing():
    D, dtype = 64, torch.bfloat16
    chunks, nl, tail = _make((1,) * 65, D, dtype)
    idx = torch.arange(8, dtype=torch.int64, device=dev())
    dst = torch.full((10, D), SENTINEL, dtype=dtype, device=dev())
    three = chunks[:3]
    rc, status = _gather(chunks, H, idx, None, 8, nl, tail, 2, dst, 10)
    assert rc == -3 and status == 0 and "65 chunks" in _ffi.last_error()          # VC2_ERR_UNSUPPORTED
    assert _gather(three, H, idx, None, 8, nl, tail, 2, dst, 10, n_chunks=0)[0] == -3
    for kw in (dict(rows=[4, 0, 4]), dict(rows=[4, 6, 4]), dict(dtype=3)):         # VC2_ERR_ARG from here on
        assert _gather(three, H, idx, None, 8, nl, tail, 2, dst, 10, **kw)[0] == -1, kw
    assert _gather(three, -1, idx, None, 8, nl, tail, 2, dst, 10)[0] == -1
    assert _gather(three, H, idx, None, 8, None, tail, 2, dst, 10)[0] == -1         # a grid without the newline
    assert _gather(three, H, idx, None, 8, nl, None, 2, dst, 10)[0] == -1           # tail rows without the tail
    assert _gather(three, H, idx, None, 8, nl, tail, -1, dst, 10)[0] == -1
    assert _gather(three, H, None, None, 8, nl, tail, 2, dst, 10)[0] == -1
    assert _gather(three, H, idx, None, -1, nl, tail, 2, dst, 10)[0] == -1
    assert _gather(three[:2] + [None], H, idx, None, 8, nl, tail, 2, dst, 10, rows=[4, 4, 4])[0] == -1
    crow = (ctypes.c_int64 * 2)(4, 4)
    assert lib().vc2_gather_rows_grid_chunks(None, crow, 2, H, D, 1, ptr(idx), None, 8, ptr(nl), ptr(tail), 2, ptr(dst), 10,
                                             None, stream_ptr(dev())) == -1
    table = (ctypes.c_void_p * 2)(chunks[0].data_ptr(), chunks[1].data_ptr())
    assert lib().vc2_gather_rows_grid_chunks(table, crow, 2, H, D, 1, ptr(idx), None, 8, ptr(nl), ptr(tail), 2, None, 10,
                                             None, stream_ptr(dev())) == -1
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())


# ---- 2. the whole pass ------------------------------------------------------------------------------------------------------

def _newline(D, dtype, seed=11):
    return torch.randn(D, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev())


def _oracle_grid(x, ref, N, h, nl):
    """The oracle's kept set through the reference's _map_grid_vid (vidcom2.py:105-115), and the stream's rows (CPU)."""
    F = x.shape[0] // N
    ks = ref["ks"].clamp(max=N)
    loc = ref["global_idx"] - torch.repeat_interleave(torch.arange(F) * N, ks)
    gidx = O.map_grid_vid(list(torch.split(loc, ks.tolist())), h)
    return gidx, _stream([x], nl.cpu(), h)[gidx]


def _assert_same(res, whole):
    assert res.K == whole.K and torch.equal(res.ks, whole.ks) and torch.equal(res.global_idx, whole.global_idx)
    assert (res.rows is None and whole.rows is None) or torch.equal(res.rows, whole.rows)


@pytest.mark.parametrize("case", [(16, 169, 512, "f16", 0.15, (7, 2, 7)), (32, 169, 512, "bf16", 0.25, (16, 16))],
                         ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[5])))
def test_grid_and_newline_equal_the_unsharded_pass_and_the_oracle(case):
    F, N, D, dn, base, frames = case
    h = 13
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 1, base, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])                             # the unsharded pass itself
    nl = _newline(D, DTYPES[dn])
    whole = vc.compress(xd, N, base, "grid_vid", h, newline=nl, want_scores=True)
    want_idx, want_rows = _oracle_grid(x, ref, N, h, nl)
    assert torch.equal(whole.global_idx.cpu(), want_idx) and torch.equal(whole.rows.cpu(), want_rows)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, N), N, base, mapper="grid_vid", grid_h=h, newline=nl, want_scores=True)
    _assert_same(res, whole)
    assert res.K == int(ref["global_idx"].numel()) + F * h and res.ks.cpu().tolist() == ref["ks"].tolist()
    assert torch.equal(res.global_idx.cpu(), want_idx) and torch.equal(res.rows.cpu(), want_rows)
    assert tuple(res.v_score.shape) == (F, N) and res.v_score.dtype == DTYPES[dn]
    if all(f % 16 == 0 for f in frames):                                          # the same bits, the scores included
        assert torch.equal(res.v_score, whole.v_score) and torch.equal(res.f_score, whole.f_score)
    # no gather: rows is None, the indices are still mapped
    res = vc.compress_chunks(_split(xd, frames, N), N, base, gather=False, mapper="grid_vid", grid_h=h, newline=nl)
    assert res.rows is None and res.v_score is None
    assert res.K == whole.K and torch.equal(res.global_idx, whole.global_idx) and torch.equal(res.ks, whole.ks)


@pytest.mark.parametrize("m", [1, 2])
def test_tail_rows_follow_the_kept_rows(m):
    F, N, D, dn, frames = 8, 49, 64, "bf16", (3, 2, 3)
    x, xd, ref, total, rows, gidx = _reference(F, N, D, dn, 2, 0.25, 4)
    assert torch.equal(gidx.cpu(), ref["global_idx"])
    tail = torch.randn(m, D, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).to(dev())
    whole = vc.compress(xd, N, 0.25, tail=tail)
    res = vc.compress_chunks(_split(xd, frames, N), N, 0.25, tail=tail)
    _assert_same(res, whole)
    assert tuple(res.rows.shape) == (res.K + m, D) and torch.equal(res.global_idx.cpu(), ref["global_idx"])
    assert torch.equal(res.rows.cpu(), torch.cat([x[ref["global_idx"]], tail.cpu()]))
    # the cached compressor takes the next call's tensor, not the first one's
    res = vc.compress_chunks(_split(xd, frames, N), N, 0.25, tail=tail + 1)
    assert torch.equal(res.rows[res.K:], tail + 1) and torch.equal(res.rows[:res.K], whole.rows[:whole.K])


@pytest.mark.parametrize("dn", ["bf16", "f16"])
def test_scores_of_16_frame_chunks_are_the_unsharded_pass_bits(dn):
    F, N, D, frames = 32, 49, 256, (16, 16)
    xd = synth.make(F, N, D, DTYPES[dn], 1, "drift").to(dev())
    whole = vc.compress(xd, N, 0.25, want_scores=True)
    cc = vc.ChunkedCompressor(frames, N, D, DTYPES[dn], dev(), 0.25, want_scores=True)
    first = cc(_split(xd, frames, N))
    _assert_same(first, whole)
    assert first.v_score.dtype == DTYPES[dn] and tuple(first.f_score.shape) == (F, N)
    assert torch.equal(first.v_score, whole.v_score) and torch.equal(first.f_score, whole.f_score)
    # the next video gets score tensors of its own
    xd2 = synth.make(F, N, D, DTYPES[dn], 2, "drift").to(dev())
    second, whole2 = cc(_split(xd2, frames, N)), vc.compress(xd2, N, 0.25, want_scores=True)
    assert second.v_score.data_ptr() != first.v_score.data_ptr()
    assert torch.equal(second.v_score, whole2.v_score) and torch.equal(second.f_score, whole2.f_score)
    assert torch.equal(first.v_score, whole.v_score) and torch.equal(first.f_score, whole.f_score)


def _assert_scores_within(res, whole, tol=1e-6):
    """fp32 scores: DESIGN.md section 3's contract (1e-6 absolute)."""
    assert res.v_score.dtype == torch.float32 and res.f_score.dtype == torch.float32
    dv = (res.v_score - whole.v_score).abs().max().item()
    df = (res.f_score - whole.f_score).abs().max().item()
    print("max |dv|", dv, "max |df|", df)
    assert dv <= tol and df <= tol


def test_fp32_scores_of_unequal_chunks_are_within_the_fp32_contract():
    F, N, D, frames = 16, 196, 1024, (5, 11)
    xd = synth.make(F, N, D, torch.float32, 1, "drift").to(dev())
    whole = vc.compress(xd, N, 0.25, want_scores=True)
    res = vc.compress_chunks(_split(xd, frames, N), N, 0.25, want_scores=True)
    _assert_same(res, whole)
    _assert_scores_within(res, whole)


def _score32_case():
    key = (16, 169, 512, "bf16", "drift", 0, None)
    (c,) = [c for c in SD.load() if (c["F"], c["N"], c["D"], c["dtype"], c["dist"], c["seed"], c["ratio"], c["mapper"],
                                      c["base"]) == key + ("linear", 0.25)]
    return c


def test_score_dtype_with_grid_newline_and_scores():
    """16 x 169 x 512 bf16 of tests/golden/score_dtype_cases.json in chunks (5, 11), scored in fp32, on the 13 x 13 grid:
    compress(cat) with the same options; the kept tokens are the recorded reference's."""
    c, frames, h = _score32_case(), (5, 11), 13
    xd = SD.make_input(c).to(dev())
    nl = _newline(c["D"], torch.bfloat16)
    kw = dict(score_dtype=torch.float32, newline=nl, want_scores=True)
    whole = vc.compress(xd, c["N"], c["base"], "grid_vid", h, **kw)
    assert whole.ks.cpu().tolist() == c["ks"] and whole.K == c["K"] + c["F"] * h
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, c["N"]), c["N"], c["base"], mapper="grid_vid", grid_h=h, **kw)
    _assert_same(res, whole)
    assert res.rows.dtype == torch.bfloat16
    _assert_scores_within(res, whole)


def test_params_with_grid_newline():
    """("rt", 12, 196, 1024, bf16) of tests/golden/pass_params_cases.json in chunks (5, 7) on the 14 x 14 grid."""
    name, F, N, D, dn, frames, h = "rt", 12, 196, 1024, "bf16", (5, 7), 14
    (c,) = [c for c in load_json("pass_params_cases.json")["cases"]
            if (c["name"], c["F"], c["N"], c["D"], c["dtype"]) == (name, F, N, D, dn)]
    xd = make_input(F, N, D, dn, c["seed"], c["dist"]).to(dev())
    p, nl = params_of(c), _newline(D, torch.bfloat16)
    whole = vc.compress(xd, N, c["base"], "grid_vid", h, newline=nl, params=p)
    assert whole.ks.cpu().tolist() == c["ks"] and whole.K == c["K"] + F * h
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = vc.compress_chunks(_split(xd, frames, N), N, c["base"], params=p, mapper="grid_vid", grid_h=h, newline=nl)
    _assert_same(res, whole)


def test_defaults_still_issue_the_plain_selection():
    """With every option at its default the driver calls what it called: vc2_select_chunks, not the `_x` form."""
    F, N, D, frames = 8, 49, 64, (3, 2, 3)
    xd = synth.make(F, N, D, torch.bfloat16, 2, "drift").to(dev())
    for kw, name in ((dict(), "vc2_select_chunks"), (dict(want_scores=True), "vc2_select_chunks"),
                     (dict(tail=torch.zeros(1, D, dtype=torch.bfloat16, device=dev())), "vc2_select_chunks_x")):
        cc = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, dev(), 0.25, **kw)
        log = []
        cc._L = _Spy(cc._L, log)
        cc(_split(xd, frames, N))
        assert [n for n, _ in log if n.startswith("vc2_select")] == [name], kw


# ---- 3. pooled chunks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,score_dtype", [("average", None), ("max", None), ("bilinear", None),
                                              ("average", torch.float32)],
                         ids=["average", "max", "bilinear", "average-scored-in-fp32"])
def test_pooled_chunks_equal_pool_stats_and_add(mode, score_dtype):
    """[8, 36, 64] bf16 at 6 x 6 -> 9 tokens per frame, chunks of 3 and 5 frames (stat blocks of one frame); the last case
    goes through the entry point's options (vc2_shard_opts)."""
    F, Hh, Ww, D, frames, N = 8, 6, 6, 64, (3, 5), 9
    img = synth.make(F, Hh * Ww, D, torch.bfloat16, 3, "drift").to(dev()).view(F, Hh * Ww, D)
    parts = [img[:3].clone(), img[3:].clone()]
    pooled = [fused.pool_stats(p, Hh, Ww, mode)[0] for p in parts]
    a = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, dev(), 0.25, score_dtype=score_dtype)
    for p in pooled:
        a.add(p.view(-1, D))
    stats_a = a._stats_all.clone()
    want = a.finish()
    b = vc.ChunkedCompressor(frames, N, D, torch.bfloat16, dev(), 0.25, score_dtype=score_dtype)
    assert (b.stages[0]._opts is not None) == (score_dtype is not None)
    log = []
    b._L = _Spy(b._L, log)
    for s in b.stages:
        s._L = _Spy(s._L, log)
    got = [b.add_pooled(p, Hh, Ww, mode) for p in parts]
    stats_b = b._stats_all.clone()
    res = b.finish()
    names = [n for n, _ in log]
    assert not any(n.startswith("vc2_chan_stats") for n in names) and names.count("vc2_pool_stats_blocks") == 2
    for g, p, f in zip(got, pooled, frames):
        assert tuple(g.shape) == (f, N, D) and not g.requires_grad and torch.equal(g, p)
    assert stats_b.dtype == torch.float64 and torch.equal(stats_b, stats_a)
    _assert_same(res, want)
    assert torch.equal(res.rows, torch.cat([p.view(-1, D) for p in pooled])[res.global_idx])
    # add and add_pooled mixed within one video
    b.add(pooled[0].view(-1, D))
    b.add_pooled(parts[1], Hh, Ww, mode)
    _assert_same(b.finish(), want)
    # a grid that does not pool to N tokens per frame is refused before anything is enqueued
    with pytest.raises(RuntimeError, match="pooling to 4 tokens"):
        b.add_pooled(torch.zeros(3, 16, D, dtype=torch.bfloat16, device=dev()), 4, 4, mode)
    assert b._chunks == []


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------

def test_gradients_of_every_chunk_the_newline_and_the_tail():
    F, N, h, D, frames, m = 4, 9, 3, 64, (1, 3), 2
    xd = synth.make(F, N, D, torch.float32, 1, "drift").to(dev())
    g0 = torch.Generator().manual_seed(6)
    nl = torch.randn(D, generator=g0).to(dev()).requires_grad_()
    tail = torch.randn(m, D, generator=g0).to(dev()).requires_grad_()
    chunks = [c.requires_grad_() for c in _split(xd, frames, N)]
    res = vc.compress_chunks(chunks, N, 0.25, mapper="grid_vid", grid_h=h, newline=nl, tail=tail)
    whole = vc.compress(xd, N, 0.25, "grid_vid", h, newline=nl.detach(), tail=tail.detach())
    _assert_same(res, whole)
    assert res.rows.requires_grad and tuple(res.rows.shape) == (res.K + m, D)
    g = torch.randn(res.rows.shape, generator=g0).to(dev())
    got = torch.autograd.grad(res.rows, chunks + [nl, tail], g)
    # torch indexing on the torch-built stream
    leaves = [c.detach().clone().requires_grad_() for c in chunks]
    nl2, tail2 = nl.detach().clone().requires_grad_(), tail.detach().clone().requires_grad_()
    out = torch.cat([_stream(leaves, nl2, h)[res.global_idx], tail2])
    assert torch.equal(out.detach(), res.rows.detach())
    want = torch.autograd.grad(out, leaves + [nl2, tail2], g)
    for a, b, c in zip(got[:2], want[:2], chunks):
        assert a.shape == c.shape and torch.equal(a, b)
    assert all(int((a != 0).any(1).sum()) > 0 for a in got[:2])       # each chunk kept rows; dropped tokens get zero rows
    assert torch.equal(got[3], want[3]) and torch.equal(got[3], g[res.K:])
    # the newline: its slots' gradient rows summed in fp32 and rounded once (torch's scatter adds them in any order)
    is_nl = res.global_idx % (h + 1) == h
    assert int(is_nl.sum()) == F * h
    assert got[2].shape == nl.shape and torch.equal(got[2], g[:res.K][is_nl].float().sum(dim=0).to(g.dtype))
    assert torch.allclose(got[2], want[2], rtol=1e-5, atol=1e-5)
    # only the newline requires grad; no graph without one
    res2 = vc.compress_chunks([c.detach() for c in chunks], N, 0.25, mapper="grid_vid", grid_h=h, newline=nl,
                              tail=tail.detach())
    assert torch.equal(torch.autograd.grad(res2.rows, [nl], g)[0], got[2])
    with torch.no_grad():
        res3 = vc.compress_chunks(chunks, N, 0.25, mapper="grid_vid", grid_h=h, newline=nl, tail=tail)
    assert res3.rows.grad_fn is None and torch.equal(res3.rows, res.rows.detach())

"""A video held as frame chunks (vidcom2_amd/chunked.py), CPU side: the argument errors (raised before any stage exists),
the driver's order of stages and exchanges with oracle-backed CPU stages injected, the delegation of a single chunk, and the
host arithmetic of the chunk table."""
import pytest
import torch

import oracle as O
import vidcom2_amd as vc
from vidcom2_amd import PassParams, chunked, synth

from _ragged_shards import DTYPES, RaggedOracleStages


class _Factory:
    """A stage factory that counts its calls (and builds the oracle-backed CPU stages)."""

    def __init__(self):
        self.calls = 0

    def __call__(self, F, N, D, dtype, base, frames, rank):
        self.calls += 1
        return RaggedOracleStages(F, N, D, dtype, base)


def _chunks(x, frames, N):
    out, f0 = [], 0
    for f in frames:
        out.append(x[f0 * N: (f0 + f) * N].clone())
        f0 += f
    return out


# ---- errors: all before anything is built or enqueued ----------------------------------------------------------------

def test_public_names():
    assert vc.compress_chunks is chunked.compress_chunks and vc.ChunkedCompressor is chunked.ChunkedCompressor


def test_empty_list_is_a_value_error():
    fac = _Factory()
    with pytest.raises(ValueError):
        vc.compress_chunks([], 49, stages_factory=fac)
    with pytest.raises(ValueError):
        vc.ChunkedCompressor([], 49, 64, torch.bfloat16, "cpu", stages_factory=fac)
    assert fac.calls == 0


def test_more_than_64_chunks_is_not_implemented():
    fac = _Factory()
    x = torch.zeros(5, 64, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError):
        vc.compress_chunks([x] * 65, 5, stages_factory=fac)
    with pytest.raises(NotImplementedError):
        vc.ChunkedCompressor([1] * 65, 5, 64, torch.bfloat16, "cpu", stages_factory=fac)
    assert fac.calls == 0
    assert chunked.MAX_CHUNKS == 64


def test_rows_not_a_multiple_of_tpf_words_the_error_like_compress():
    fac = _Factory()
    a, b = torch.zeros(3 * 49, 64, dtype=torch.bfloat16), torch.zeros(2 * 49 + 1, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError) as e:
        vc.compress_chunks([a, b], 49, stages_factory=fac)
    assert str(e.value) == f"shape '[-1, 49, 32]' is invalid for input of size {(2 * 49 + 1) * 32}"
    with pytest.raises(RuntimeError) as e:                              # (the channel count follows params, as in compress)
        vc.compress_chunks([a, b], 49, params=PassParams(0.25), stages_factory=fac)
    assert str(e.value) == f"shape '[-1, 49, 16]' is invalid for input of size {(2 * 49 + 1) * 16}"
    assert fac.calls == 0


@pytest.mark.parametrize("kind", ["D", "dtype", "dim"])
def test_a_chunk_of_another_kind_is_a_runtime_error(kind):
    fac = _Factory()
    a = torch.zeros(3 * 49, 64, dtype=torch.bfloat16)
    b = {"D": torch.zeros(2 * 49, 128, dtype=torch.bfloat16), "dtype": torch.zeros(2 * 49, 64, dtype=torch.float16),
         "dim": torch.zeros(2, 49, 64, dtype=torch.bfloat16)}[kind]
    with pytest.raises(RuntimeError, match="chunk 1 must be a torch.bfloat16"):
        vc.compress_chunks([a, b], 49, stages_factory=fac)
    assert fac.calls == 0


def test_a_frame_count_that_disagrees_with_the_layout_is_a_runtime_error():
    fac = _Factory()
    cc = vc.ChunkedCompressor([3, 2], 49, 64, torch.bfloat16, "cpu", stages_factory=fac)
    built = fac.calls
    with pytest.raises(RuntimeError, match=r"chunk 0 must be a torch.bfloat16 \[147, 64\] tensor"):
        cc.add(torch.zeros(2 * 49, 64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="chunk 1 must be"):          # (the whole list is checked before the first add)
        cc([torch.zeros(3 * 49, 64, dtype=torch.bfloat16), torch.zeros(3 * 49, 64, dtype=torch.bfloat16)])
    assert fac.calls == built and cc._chunks == [] and cc._pending is None


def test_bad_params_and_score_dtype_raise_what_hip_stages_raises():
    fac = _Factory()
    a = torch.zeros(3 * 49, 64, dtype=torch.bfloat16)
    for kw, err in ((dict(params="0.5"), TypeError), (dict(params=PassParams(0.001)), ValueError),
                    (dict(score_dtype=torch.float16), ValueError)):
        with pytest.raises(err):
            vc.compress_chunks([a, a], 49, stages_factory=fac, **kw)
        with pytest.raises(err):
            vc.ChunkedCompressor([3, 3], 49, 64, torch.bfloat16, "cpu", stages_factory=fac, **kw)
    with pytest.raises(NotImplementedError):                            # more scored channels than the sweeps take
        vc.ChunkedCompressor([3, 3], 49, 8192, torch.bfloat16, "cpu", params=PassParams(0.75), stages_factory=fac)
    with pytest.raises(ValueError):
        vc.ChunkedCompressor([3, 0], 49, 64, torch.bfloat16, "cpu", stages_factory=fac)
    assert fac.calls == 0


def test_finish_before_the_last_chunk_and_an_extra_chunk():
    cc = vc.ChunkedCompressor([1, 1], 5, 64, torch.bfloat16, "cpu", stages_factory=_Factory())
    x = synth.make(2, 5, 64, torch.bfloat16, 1, "drift")
    cc.add(x[:5])
    with pytest.raises(RuntimeError, match="1 of 2 chunks"):
        cc.finish()
    cc.add(x[5:])
    with pytest.raises(RuntimeError, match="added already"):
        cc.add(x[5:])
    assert cc.finish().ks.numel() == 2


# ---- the driver on the CPU --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(8, 49, 64, "bf16", (3, 2, 3)), (12, 5, 128, "f16", (5, 1, 1, 5))],
                         ids=lambda c: "x".join(map(str, c[:4])) + "-" + "+".join(map(str, c[4])))
def test_driver_with_oracle_stages_matches_the_oracle(case):
    """The order of stages and exchanges of the chunk driver with the oracle-backed CPU stages: budgets and kept indices
    are the whole-pass oracle's, the rows those of the virtual concatenation."""
    F, N, D, dn, frames = case
    assert sum(frames) == F and min(frames) >= 1
    x = synth.make(F, N, D, DTYPES[dn], 3, "drift")
    ref = O.compress_indices(x, N, 0.25)
    fac = _Factory()
    res = vc.compress_chunks(_chunks(x, frames, N), N, 0.25, stages_factory=fac)
    assert fac.calls == len(frames)
    assert res.ks.tolist() == ref["ks"].tolist()
    assert torch.equal(res.global_idx, ref["global_idx"]) and res.K == ref["global_idx"].numel()
    assert torch.equal(res.rows, x[ref["global_idx"]])
    # the compressor object, chunk by chunk, twice (reuse)
    cc = vc.ChunkedCompressor(frames, N, D, DTYPES[dn], "cpu", 0.25, gather=False, stages_factory=fac)
    for _ in range(2):
        for c in _chunks(x, frames, N):
            cc.add(c)
        got = cc.finish()
        assert got.rows is None and torch.equal(got.global_idx, ref["global_idx"])


def test_one_chunk_delegates_to_compress(monkeypatch):
    seen = {}

    def fake(x, tpf, base_scale=0.25, **kw):
        seen.update(x=x, tpf=tpf, base=base_scale, kw=kw)
        return "delegated"
    monkeypatch.setattr(chunked._vc, "compress", fake)
    x = torch.zeros(3 * 49, 64, dtype=torch.bfloat16)
    p = PassParams(0.25)
    assert vc.compress_chunks([x], 49, 0.3, gather=False, params=p, score_dtype=torch.float32) == "delegated"
    assert seen["x"] is x and seen["tpf"] == 49 and seen["base"] == 0.3
    assert seen["kw"] == dict(gather=False, params=p, score_dtype=torch.float32)


# ---- the chunk table ----------------------------------------------------------------------------------------------------

def test_chunk_table_prefix_sums_and_owners():
    rows = [3 * 49, 1 * 49, 7 * 49, 49]
    starts = chunked.chunk_starts(rows)
    assert starts == [0, 147, 196, 539, 588]
    assert chunked.chunk_of_row(starts, 0) == 0 and chunked.chunk_of_row(starts, starts[-1] - 1) == len(rows) - 1
    for c in range(1, len(rows)):
        assert chunked.chunk_of_row(starts, starts[c] - 1) == c - 1
        assert chunked.chunk_of_row(starts, starts[c]) == c
    for bad in (-1, starts[-1]):
        with pytest.raises(IndexError):
            chunked.chunk_of_row(starts, bad)
    with pytest.raises(ValueError):
        chunked.chunk_starts([5, 0, 5])
    ones = chunked.chunk_starts([1] * 64)                               # 64 chunks of one row
    assert ones == list(range(65)) and [chunked.chunk_of_row(ones, r) for r in (0, 31, 63)] == [0, 31, 63]
    cc = vc.ChunkedCompressor([3, 1, 7, 1], 49, 64, torch.bfloat16, "cpu", stages_factory=_Factory())
    assert cc.starts == starts and cc.f0s == [0, 3, 4, 11] and cc.F_total == 12

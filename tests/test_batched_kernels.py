"""vc2_keep_positions_batched / vc2_repad_rows against their torch definition (models/_prefill_prune.py
`_batched_layout`), bit for bit, and `compress_batch` with one tokens-per-frame value per clip."""
import pytest
import torch

from vidcom2_amd import synth

pytestmark = pytest.mark.gpu


def _case(B, S, seed, kind="random"):
    g = torch.Generator().manual_seed(seed)
    vm = torch.rand((B, S), generator=g) < 0.6
    if kind == "all_video":
        vm[:] = True
    if B > 1:
        vm[B - 1] = False                                      # a row without video tokens
    if kind == "all_video" and B > 1:
        vm[0] = True
    nvid = int(vm.sum())
    frac = 0.0 if kind == "k0" else 0.3
    kept = torch.nonzero(torch.rand(nvid, generator=g) < frac).squeeze(-1)
    return g, vm, kept


def _padded_mask(g, B, S, left):
    am = torch.ones((B, S), dtype=torch.int64)
    for b in range(B):
        npad = int(torch.randint(0, max(1, S // 4), (1,), generator=g)) if S > 1 and b % 2 == 0 else 0
        if npad:
            if left:
                am[b, :npad] = 0
            else:
                am[b, S - npad:] = 0
    return am


@pytest.mark.parametrize("kind", ["random", "all_video", "k0"])
@pytest.mark.parametrize("left", [True, False])
@pytest.mark.parametrize("B,S", [(1, 1), (1, 300), (2, 17), (3, 1000), (8, 4096), (2, 70000), (3, 1 << 17)])
def test_keep_positions_batched_matches_definition(B, S, left, kind):
    from vidcom2_amd.fused import keep_positions_batched
    from vidcom2_amd.models._prefill_prune import _batched_layout
    g, vm, kept = _case(B, S, S * 31 + B, kind)
    am = _padded_mask(g, B, S, left)
    vpm = vm | (torch.rand((B, S), generator=g) < 0.1)
    pos = torch.randint(0, 1 << 20, (4, B, S), generator=g)
    ref = _batched_layout(vm, kept, left, am, pos, True, vpm)
    dev = "cuda"
    got = keep_positions_batched(vm.to(dev), kept.to(dev), int(vm.sum()), left, vpm.to(dev), am.to(dev), pos.to(dev),
                                 True, int(vpm.sum()))
    assert got.S == ref.S
    assert torch.equal(got.keep.cpu(), ref.keep)
    assert torch.equal(got.lengths.cpu(), ref.lengths)
    assert torch.equal(got.mask.cpu(), ref.mask)
    assert torch.equal(got.pos.cpu(), ref.pos)
    assert torch.equal(got.vis_rows.cpu(), ref.vis_rows)
    # without the optional outputs, 3 position planes, no text row
    ref3 = _batched_layout(vm, kept, left, None, pos[1:], False, None)
    got3 = keep_positions_batched(vm.to(dev), kept.to(dev), None, left, None, None, pos[1:].to(dev), False)
    assert torch.equal(got3.keep.cpu(), ref3.keep) and torch.equal(got3.pos.cpu(), ref3.pos)
    assert got3.mask is None and got3.vis_rows is None


def test_keep_positions_batched_errors_raise():
    from vidcom2_amd.fused import keep_positions_batched
    dev = "cuda"
    vm = torch.zeros((2, 64), dtype=torch.bool)
    vm[0, 10:30] = True
    vm[1, 5:9] = True
    kept = torch.tensor([1, 3, 20, 22])
    vmd = vm.to(dev)
    keep_positions_batched(vmd, kept.to(dev), 24)                          # sound
    with pytest.raises(IndexError, match="ascending"):
        keep_positions_batched(vmd, torch.tensor([3, 1], device=dev), 24)
    with pytest.raises(IndexError, match="ascending"):
        keep_positions_batched(vmd, torch.tensor([1, 24], device=dev), 24)   # beyond the batch's video positions
    with pytest.raises(IndexError, match="different number"):
        keep_positions_batched(vmd, kept.to(dev), 25)
    vis = torch.zeros_like(vm)
    with pytest.raises(IndexError, match="not flagged"):
        keep_positions_batched(vmd, kept.to(dev), 24, visual_mask=vis.to(dev), n_visual=0)
    with pytest.raises(IndexError, match="visual rows"):
        keep_positions_batched(vmd, kept.to(dev), 24, visual_mask=vmd, n_visual=2)   # capacity of 2 rows
    # the stream is sound afterwards
    got = keep_positions_batched(vmd, kept.to(dev), 24)
    assert got.lengths.tolist() == [64 - 20 + 2, 64 - 4 + 2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 1024, 3584, 4096, 1001])
def test_repad_rows_matches_definition(D, dtype):
    from vidcom2_amd.fused import repad_rows
    from vidcom2_amd.models._prefill_prune import _gather_slots
    B, S = 3, 257
    g = torch.Generator().manual_seed(D)
    src = synth.to_torch(synth.gauss(D, 50, 0, B * S * D).reshape(B, S, D), dtype)
    Sp = 200
    keep = torch.randint(0, S, (B, Sp), generator=g)
    keep[0, :13] = -1
    keep[2, 150:] = -1
    ref = _gather_slots(src, keep, 0)
    got = repad_rows(src.cuda(), keep.cuda(), check=True)
    assert torch.equal(got.cpu(), ref)
    # an unaligned view (odd row offset) takes the element path
    got2 = repad_rows(src.cuda()[:, 1:], (keep.clamp(max=S - 2)).cuda())
    assert torch.equal(got2.cpu(), _gather_slots(src[:, 1:], keep.clamp(max=S - 2), 0))


def test_repad_rows_out_of_range_is_reported_not_read():
    from vidcom2_amd.fused import repad_rows
    src = torch.ones((2, 8, 64), dtype=torch.bfloat16, device="cuda")
    keep = torch.tensor([[0, 7, 8], [1, -1, 1 << 40]], device="cuda")
    with pytest.raises(IndexError):
        repad_rows(src, keep, check=True)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = repad_rows(src, keep, status=st)
    assert int(st.item()) & 2
    assert out[0, 2].abs().sum().item() == 0 and out[1, 2].abs().sum().item() == 0 and out[0, 1].sum().item() == 64


def test_compress_batch_per_clip_tpf():
    import vidcom2_amd as vc
    clips = [synth.make(8, 36, 128, torch.bfloat16, seed=1, dist="drift"),
             synth.make(6, 48, 128, torch.bfloat16, seed=2, dist="drift"),
             synth.make(8, 36, 128, torch.bfloat16, seed=3, dist="drift"),
             synth.make(4, 64, 128, torch.bfloat16, seed=4, dist="drift")]
    tpfs = [36, 48, 36, 64]
    got = vc.compress_batch([c.cuda() for c in clips], tpfs, 0.25, gather=False)
    for c, t, r in zip(clips, tpfs, got):
        one = vc.compress(c.cuda(), t, 0.25, gather=False)
        assert r.K == one.K and torch.equal(r.global_idx, one.global_idx) and torch.equal(r.ks, one.ks)
    with pytest.raises(ValueError):
        vc.compress_batch([c.cuda() for c in clips], tpfs[:2])

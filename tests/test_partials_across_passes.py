"""The sweeps' partials (sweep 1's per-group channel sums, sweep 2's block sums and column sums) live in ONE workspace
per plan and are rewritten by every pass, with write-through stores that leave the writer's L2 as they are issued.  What a
cache-policy change could break and no other test aims at: a reader that sees the PREVIOUS pass's partials.  Two
different clips of the same shape go alternately through one plan (same workspace, same stream) for a few dozen passes;
every pass must return exactly what a fresh plan returns for that clip: budgets, kept indices, kept rows."""
import pytest
import torch

from vidcom2_amd import synth

pytestmark = pytest.mark.gpu
PASSES = 36
SHAPES = [(8, 196, 3584), (16, 169, 3584), (6, 324, 3584), (128, 196, 3584)]      # the last one: the target shape


def _snapshot(r):
    return r.ks.clone(), r.global_idx.clone(), r.rows.clone()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_alternating_clips_through_one_plan(shape, dt):
    from vidcom2_amd.vidcom2 import CompressPlan
    F, N, D = shape
    dev = torch.device("cuda:0")
    clips = [synth.make(F, N, D, dt, 7100, "drift").to(dev), synth.make(F, N, D, dt, 7101, "iid").to(dev)]
    want = []
    for x in clips:                                     # a fresh plan (its own workspace) per clip
        fresh = CompressPlan(F, N, D, dt, dev, 0.25)
        fresh.enqueue(x)
        want.append(_snapshot(fresh.finish()))
        torch.cuda.synchronize()
    assert not (torch.equal(want[0][0], want[1][0]) and torch.equal(want[0][1], want[1][1])), "the two clips must differ"
    plan = CompressPlan(F, N, D, dt, dev, 0.25)
    bad = []
    for i in range(PASSES):
        which = i & 1
        plan.enqueue(clips[which])
        ks, idx, rows = _snapshot(plan.finish())
        if not (torch.equal(ks, want[which][0]) and torch.equal(idx, want[which][1]) and torch.equal(rows, want[which][2])):
            bad.append(i)
    torch.cuda.synchronize()
    assert not bad, f"passes {bad} of {PASSES} differ from a fresh plan's result at {shape} {dt}"

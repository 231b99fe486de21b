"""Batched Qwen-VL prompts for the batched-prefill tests (test infrastructure): rows derived from a
`hook_cases.json` case (same feature size, dtype and retention ratio -- R_RATIO is one knob for the whole batch) with
their own prompt lengths, seeds and video counts, padded on the left or the right to one length."""
from __future__ import annotations

import torch

import _stub_models as S

PAD_ID = 0


def row_cases(c, n_rows: int, with_empty: bool = True):
    """n_rows variants of case `c`: every row its own seed and text lengths; the video count varies (all of the case's
    videos, the first one only, ...) and, with_empty, the last row carries no video at all."""
    rows = []
    for i in range(n_rows):
        r = dict(c)
        r["seed"] = c["seed"] + 1000 * i
        r["prefix"] = c["prefix"] + 3 * i
        r["suffix"] = c["suffix"] + (5 * i) % 7
        r["grids"] = c["grids"] if i % 2 == 0 else c["grids"][:1]
        r["n_image"] = 0
        if with_empty and i == n_rows - 1 and n_rows > 1:
            r["grids"] = []
        rows.append(r)
    return rows


def single_inputs(r):
    """(ids [1, L], per-video features, grids) of one row."""
    ids, feats, _, _ = S.qwen_inputs({**r, "mask": "none"})
    return ids, feats, [list(g) for g in r["grids"]]


def batch_inputs(rows, side: str = "left"):
    """ids [B, S] (pad id 0), per-video features in row order, grids in row order, attention mask [B, S] int64, and
    the valid lengths -- rows padded on `side` ("left" / "right")."""
    singles = [single_inputs(r) for r in rows]
    L = max(s[0].shape[1] for s in singles)
    ids = torch.full((len(rows), L), PAD_ID, dtype=torch.int64)
    mask = torch.zeros((len(rows), L), dtype=torch.int64)
    feats, grids, lens = [], [], []
    for b, (i, f, g) in enumerate(singles):
        n = i.shape[1]
        sl = slice(L - n, L) if side == "left" else slice(0, n)
        ids[b, sl] = i[0]
        mask[b, sl] = 1
        feats += f
        grids += g
        lens.append(n)
    return ids, feats, grids, mask, lens


def text_positions(mask):
    """What generate gives a padded batch as text positions: cumsum - 1, 0 at pad slots."""
    return torch.where(mask != 0, mask.cumsum(1) - 1, torch.zeros((), dtype=torch.int64))


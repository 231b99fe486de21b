"""Prefill pruning shared by the Qwen-VL hooks.

What the reference's patched forwards do between "video embeddings scattered into the prompt"
and "language model called" (models/qwen2_5_vl.py:126-185, models/qwen2_vl.py:101-147), as an
interceptor around the model's own forward:

1. `get_placeholder_mask` is watched to learn where the video placeholders sit and which
   embeddings were scattered there (the model's own call, nothing recomputed);
2. the call into `self.language_model` is intercepted: kept video positions are decided by
   `choose(video_embeds)`, then `inputs_embeds`, `attention_mask` (2-D or 4-D) and
   `position_ids` are sliced to text + kept video positions and the real language model runs.

Position ids are computed by the model before the language-model call, i.e. on the *unpruned*
sequence, which is what the reference does on purpose (qwen2_5_vl.py:89: "Pre-compute position
ids before pruning so we can safely slice them later").

Batches of B > 1 prompts (`VC2_BATCHED_PREFILL=1`; the reference leaves them unpruned): every row is pruned exactly as
the batch-1 path prunes that prompt alone -- its non-video positions, padding included, plus its kept video tokens --
and the rows, now of different lengths n_b, are re-padded to S' = max n_b on the side the batch was padded on (new pad
slots: mask 0, zero embedding, the row's pad position value).  `_batched_layout` is the executable definition; the
device path (`fused.keep_positions_batched` + `fused.repad_rows`) reproduces it bit for bit.  `generate()` keeps growing
the UNPRUNED mask during the decode steps that follow, while the KV cache holds the pruned layout: `run_decode_step`
maps the mask that reaches the language model onto that layout (the positions need no change: generate derives them
from the unpruned mask and `rope_deltas`, i.e. from each row's valid length, as for the row alone).

`renumber=True` (the transformers LLaVA hooks, `llava_hf.py`) is the other position contract: the reference prunes LLaVA
prompts BEFORE positions exist, so the pruned prompt is numbered 0 .. S'-1 and decoding continues at S'.  A 2-D
`position_ids [B, S]` then leaves with every kept position lowered by the number of that row's dropped tokens before it
(B > 1: the batched layout's `text_row0` plane), absent positions stay absent, and the decode layout carries the row's
dropped count, which `run_decode_step` subtracts from the positions generate derives from the unpruned mask.
"""
from __future__ import annotations

import warnings
from typing import Callable, NamedTuple, Optional

import torch

from ._intercept import batched_prefill_enabled, shadow


class PruneState:
    """Filled while the wrapped forward runs; read by tests through `model._vidcom2_last`."""

    def __init__(self) -> None:
        self.video_mask: Optional[torch.Tensor] = None       # [B, S] bool
        self.video_embeds: Optional[torch.Tensor] = None     # [n_video_tokens, D]
        self.kept_video: Optional[torch.Tensor] = None       # sorted indices into the video tokens
        self.keep_token_indices: Optional[torch.Tensor] = None   # sorted positions in the sequence ([B, S'] for B > 1,
        #                                                         -1 in pad slots)
        self.lengths: Optional[torch.Tensor] = None              # [B] kept positions per row
        self.pruned = False
        self.decode: Optional["_DecodeLayout"] = None            # (B > 1) what the decode steps need


class _DecodeLayout(NamedTuple):
    mask: torch.Tensor          # [B, S'] pruned 2-D mask of the prefill
    keep: torch.Tensor          # [B, S'] kept positions (-1: pad slot)
    S: int                      # unpruned prompt length
    dropped: Optional[torch.Tensor] = None      # [B] tokens dropped per row (renumbered positions only)


_WARNED: set = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _WARNED:
        _WARNED.add(key)
        warnings.warn(msg, RuntimeWarning, stacklevel=4)


class BatchedLayout(NamedTuple):
    """The pruned, re-padded layout of a batch (what `fused.keep_positions_batched` returns on the device)."""
    keep: torch.Tensor                      # int64 [B, S'], -1 in pad slots
    lengths: torch.Tensor                   # int64 [B]
    S: int                                  # S'
    vis_rows: Optional[torch.Tensor]        # int64, ordinals among the flattened visual positions
    mask: Optional[torch.Tensor]            # int64 [B, S']
    pos: Optional[torch.Tensor]             # int64 [R, B, S']


def _batched_layout(vm: torch.Tensor, kept: torch.Tensor, pad_left: bool, am: Optional[torch.Tensor] = None,
                    pos: Optional[torch.Tensor] = None, text_row0: bool = False,
                    vpm: Optional[torch.Tensor] = None) -> BatchedLayout:
    """Definition of the batched keep list (torch indexing; include/vc2.h vc2_keep_positions_batched): vm [B, S] bool,
    kept = ascending ordinals over the batch's video positions in row-major order, am [B, S] int64, pos [R, B, S] int64,
    vpm [B, S] bool."""
    B, S = vm.shape
    dev = vm.device
    flags = torch.zeros(int(vm.sum()), dtype=torch.bool, device=dev)
    flags[kept.to(dev)] = True
    keep_flags = ~vm
    keep_flags[vm] = flags
    lengths = keep_flags.sum(1)
    Sp = int(lengths.max())
    keep = torch.full((B, Sp), -1, dtype=torch.int64, device=dev)
    for b in range(B):
        idx = keep_flags[b].nonzero(as_tuple=False).squeeze(-1)
        off = Sp - idx.numel() if pad_left else 0
        keep[b, off:off + idx.numel()] = idx
    slot = keep >= 0
    kc = keep.clamp(min=0)
    mask = out_pos = vis_rows = None
    if am is not None:
        mask = torch.where(slot, am.gather(1, kc), torch.zeros((), dtype=am.dtype, device=dev))
    if pos is not None:
        R = pos.shape[0]
        if am is not None:
            pad = am == 0
            fpad = torch.where(pad.any(1), pad.to(torch.int64).argmax(1), torch.full_like(lengths, -1))
        else:
            fpad = torch.full_like(lengths, -1)
        fill = torch.where(fpad >= 0, pos.gather(2, fpad.clamp(min=0).view(1, B, 1).expand(R, B, 1))[..., 0],
                           torch.zeros((), dtype=pos.dtype, device=dev))          # [R, B]
        out_pos = torch.where(slot, pos.gather(2, kc.expand(R, B, Sp)), fill[..., None])
        if text_row0:
            valid = slot & (mask != 0) if mask is not None else slot
            out_pos[0] = torch.where(valid, valid.to(torch.int64).cumsum(1) - 1, fill[0][:, None])
    if vpm is not None:
        vis_rows = (vpm.reshape(-1).to(torch.int64).cumsum(0) - 1)[(keep_flags & vpm).reshape(-1)]
    return BatchedLayout(keep, lengths, Sp, vis_rows, mask, out_pos)


def _gather_slots(t: torch.Tensor, keep: torch.Tensor, fill) -> torch.Tensor:
    """t[b, keep[b, j]] along dim 1 of a [B, S, ...] tensor, `fill` where keep < 0."""
    kc = keep.clamp(min=0).view(keep.shape + (1,) * (t.dim() - 2)).expand(keep.shape + t.shape[2:])
    slot = (keep >= 0).view(keep.shape + (1,) * (t.dim() - 2))
    return torch.where(slot, t.gather(1, kc), torch.full((), fill, dtype=t.dtype, device=t.device))


def _padding_side(am) -> Optional[bool]:
    """True = left, False = right, None = neither (a 2-D mask); no mask / all ones: left."""
    if am is None:
        return True
    ends, starts = torch.stack(((am[:, -1] != 0).all(), (am[:, 0] != 0).all())).tolist()
    return True if ends else (False if starts else None)


def _map_decode_mask(am, dec: _DecodeLayout, past: int, q: int, B: int):
    """The mask generate built for the UNPRUNED prompt + t new tokens, mapped onto the pruned layout of the KV cache:
    the prefill's pruned mask followed by the columns generate appended."""
    mask, keep = dec.mask, dec.keep
    if mask.shape[0] != B:
        if B % mask.shape[0]:
            return am
        mask, keep = mask.repeat_interleave(B // mask.shape[0], 0), keep.repeat_interleave(B // keep.shape[0], 0)
    Sp = mask.shape[1]
    if am is None:
        extra = past + q - Sp
        return torch.cat((mask, torch.ones((B, extra), dtype=mask.dtype, device=mask.device)), 1) if extra >= 0 else None
    if isinstance(am, dict):
        return {k: _map_decode_mask(v, dec, past, q, B) for k, v in am.items()}
    if not torch.is_tensor(am) or am.shape[-1] < dec.S:
        return am
    if am.dim() == 2:
        return torch.cat((mask.to(device=am.device, dtype=am.dtype), am[:, dec.S:]), 1)
    if am.dim() == 4:
        t = am.shape[-1] - dec.S
        cols = torch.cat((keep.to(am.device), torch.arange(dec.S, dec.S + t, device=am.device).expand(B, t)), 1)
        kc = cols.clamp(min=0)[:, None, None, :].expand(am.shape[0], am.shape[1], am.shape[2], cols.shape[1])
        out = am.gather(3, kc)
        off = torch.zeros((), dtype=am.dtype, device=am.device) if am.dtype == torch.bool else \
            torch.full((), torch.finfo(am.dtype).min, dtype=am.dtype, device=am.device)
        return torch.where((cols >= 0)[:, None, None, :], out, off)
    return am


def _prune_attention(attn, keep: torch.Tensor):
    if not torch.is_tensor(attn):
        return attn
    if attn.dim() == 2:
        return attn[:, keep]
    if attn.dim() == 4:
        return attn[:, :, keep, :][:, :, :, keep]
    return attn


def _fusable(embeds, kept, video_embeds, deep) -> bool:
    """The device kernels take one GPU, fp32 / bf16 / fp16 rows and (deep-stack) up to 8 same-shaped tensors."""
    if not (embeds.is_cuda and torch.is_tensor(kept) and kept.is_cuda and torch.is_tensor(video_embeds)):
        return False
    if embeds.dtype not in (torch.float32, torch.bfloat16, torch.float16) or embeds.dim() != 3:
        return False
    if deep is not None:
        deep = list(deep)
        if len(deep) > 8 or any((not torch.is_tensor(d)) or d.dim() != 2 or d.device != embeds.device
                                or d.dtype != deep[0].dtype or d.shape != deep[0].shape for d in deep):
            return False
        if deep and deep[0].dtype not in (torch.float32, torch.bfloat16, torch.float16):
            return False
    return True


class _LanguageModelShim:
    """Stands in for `self.language_model` during one forward; everything but the call itself
    (attributes, sub-modules, config) is the real module's."""

    def __init__(self, real, state: PruneState, choose: Callable[[torch.Tensor], Optional[torch.Tensor]],
                 choose_many: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, renumber: bool = False):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_state", state)
        object.__setattr__(self, "_choose", choose)
        object.__setattr__(self, "_choose_many", choose_many)
        object.__setattr__(self, "_renumber", renumber)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_real"), name)

    def __call__(self, *args, **kwargs):
        st: PruneState = self._state
        embeds = kwargs.get("inputs_embeds")
        if st.video_mask is not None and torch.is_tensor(embeds) and embeds.shape[0] == 1:
            kept = self._choose(st.video_embeds)
            if kept is not None:
                vm = st.video_mask[0].to(embeds.device)
                vpm = kwargs.get("visual_pos_masks")
                deep = kwargs.get("deepstack_visual_embeds") if torch.is_tensor(vpm) else None
                fused = _fusable(embeds, kept, st.video_embeds, deep) and vm.numel() == embeds.shape[1]
                vis_rows = None
                if fused:
                    # device-side keep list + ONE launch for text rows and kept video rows (vc2_keep_positions,
                    # vc2_gather_scatter): no nonzero() round trips
                    from ..fused import gather_scatter, keep_positions
                    n_video = int(st.video_embeds.shape[0])
                    want_vis = deep is not None and len(deep) > 0
                    keep, vis_rows = keep_positions(vm, kept, n_video, vpm[0].to(embeds.device) if want_vis else None,
                                                    int(deep[0].shape[0]) if want_vis else None)
                    keep_flags = None
                    # (no second read-back: keep_positions has just validated the list -- strictly ascending positions of
                    #  a mask as long as `embeds` -- and raised otherwise; vis_rows likewise against the deep-stack rows)
                    kwargs["inputs_embeds"] = gather_scatter([embeds[0]], keep, check=False)[0][None]
                else:
                    video_pos = vm.nonzero(as_tuple=False).squeeze(-1)
                    keep_flags = ~vm
                    keep_flags[video_pos[kept]] = True
                    keep = keep_flags.nonzero(as_tuple=False).squeeze(-1)
                    kwargs["inputs_embeds"] = embeds[:, keep, :]
                if torch.is_tensor(kwargs.get("input_ids")):
                    kwargs["input_ids"] = kwargs["input_ids"][:, keep]
                if "attention_mask" in kwargs:
                    am = kwargs["attention_mask"]
                    kwargs["attention_mask"] = ({k: _prune_attention(v, keep) for k, v in am.items()}
                                                if isinstance(am, dict) else _prune_attention(am, keep))
                pos = kwargs.get("position_ids")
                if self._renumber:
                    if torch.is_tensor(pos) and pos.dim() == 2:
                        # the pruned prompt is numbered as if the dropped tokens had never been there
                        kp = keep.to(pos.device)
                        before = kp - torch.arange(kp.numel(), device=kp.device)
                        kwargs["position_ids"] = pos[:, kp] - before.to(pos.dtype)
                elif torch.is_tensor(pos):
                    pos = pos[..., keep.to(pos.device)]
                    if pos.dim() == 3 and pos.shape[0] == 4:
                        # transformers >= 4.5x prepends a row of TEXT positions that the decoder only uses to
                        # detect packed sequences (any step != 1 starts a new one).  The gaps left by the dropped
                        # video tokens must not read as packing: the kept prompt is one sequence.
                        pos = pos.clone()
                        pos[0] = torch.arange(pos.shape[-1], device=pos.device, dtype=pos.dtype).expand_as(pos[0])
                    kwargs["position_ids"] = pos
                elif pos is None and "position_ids" in kwargs:
                    # the model could not build 3-D positions and leaves them to the decoder, which would number
                    # the PRUNED prompt 0..S'-1.  The reference computes positions before pruning and slices them
                    # (qwen2_5_vl.py:89-118): do the same with the plain positions of the full prompt.
                    rope = keep.view(1, 1, -1).expand(3, embeds.shape[0], -1)
                    text = torch.arange(keep.numel(), device=keep.device).view(1, 1, -1).expand(1, embeds.shape[0], -1)
                    kwargs["position_ids"] = torch.cat((text, rope), dim=0)
                cp = kwargs.get("cache_position")
                if torch.is_tensor(cp) and cp.dim() == 1 and cp.numel() == embeds.shape[1]:
                    kwargs["cache_position"] = cp[: keep.numel()]       # prefill: slots 0 .. S'-1 of the KV cache
                # Qwen3-VL deepstack: per-layer features of the visual tokens, row i <-> i-th True of the mask
                # (models/qwen3_vl.py:141-149, 200-226 of the reference)
                if torch.is_tensor(vpm):
                    if vis_rows is not None:
                        # the deep-stack tensors share ONE index list: one launch for all of them
                        kwargs["deepstack_visual_embeds"] = gather_scatter(list(deep), vis_rows, check=False)
                    else:
                        if keep_flags is None:
                            keep_flags = torch.zeros(vm.numel(), dtype=torch.bool, device=keep.device)
                            keep_flags[keep] = True
                        rows = keep_flags[vpm[0].to(keep_flags.device)]
                        deep_any = kwargs.get("deepstack_visual_embeds")
                        if deep_any is not None:
                            kwargs["deepstack_visual_embeds"] = [d[rows.to(d.device)] for d in deep_any]
                    kwargs["visual_pos_masks"] = vpm[:, keep.to(vpm.device)]
                st.kept_video, st.keep_token_indices, st.pruned = kept, keep, True
                st.lengths = torch.tensor([keep.numel()])
        elif (st.video_mask is not None and torch.is_tensor(embeds) and embeds.shape[0] > 1
              and self._choose_many is not None and batched_prefill_enabled()):
            self._prune_batch(kwargs, embeds)
        return self._real(*args, **kwargs)

    def _prune_batch(self, kwargs: dict, embeds: torch.Tensor) -> None:
        """B > 1: every row pruned as the batch-1 path prunes it alone, re-padded to S' (module docstring)."""
        st: PruneState = self._state
        B, S = embeds.shape[:2]
        am = kwargs.get("attention_mask")
        if am is not None and not (torch.is_tensor(am) and am.dim() == 2 and tuple(am.shape) == (B, S)):
            _warn_once("mask", "vidcom2: batched prefill pruning needs a 2-D attention mask (or none); this batch of "
                       f"{B} prompts runs unpruned")
            return
        pad_left = _padding_side(am)
        if pad_left is None:
            _warn_once("side", "vidcom2: the attention mask is neither left- nor right-padded; this batch of "
                       f"{B} prompts runs unpruned")
            return
        vm = st.video_mask.to(embeds.device)
        if tuple(vm.shape) != (B, S):
            return
        kept = self._choose_many(st.video_embeds)
        am_dtype = am.dtype if am is not None else torch.int64
        am64 = am.to(torch.int64) if am is not None else torch.ones((B, S), dtype=torch.int64, device=embeds.device)
        vpm = kwargs.get("visual_pos_masks")
        vpm = vpm.to(embeds.device).bool() if torch.is_tensor(vpm) else None
        deep = kwargs.get("deepstack_visual_embeds") if vpm is not None else None
        pos = kwargs.get("position_ids")
        pos_in, text_row0, squeeze, as_bits = None, False, False, False
        if torch.is_tensor(pos):
            pos_in = pos.to(embeds.device)
            if pos_in.dim() == 2:
                pos_in, squeeze = pos_in[None], True
            text_row0 = pos_in.shape[0] == 4 or (self._renumber and squeeze)
            if pos_in.is_floating_point() and not text_row0:
                # Qwen3-Omni's TMRoPE positions are fp32 and may be fractional.  Without text_row0 the layout only copies
                # position values (pad value 0 = the bits of 0.0), so they travel exactly as the 64-bit words of an fp64
                pos_in, as_bits = pos_in.to(torch.float64).view(torch.int64), True
        elif pos is None and "position_ids" in kwargs and not self._renumber:
            # the positions the batch-1 path builds for the row alone (text 0.., rope = position in the unpadded row)
            base = torch.where(am64 != 0, am64.cumsum(1) - 1, torch.zeros((), dtype=torch.int64, device=embeds.device))
            pos_in, text_row0 = base[None].expand(4, B, S), True
        want_vis = vpm is not None and deep is not None and len(deep) > 0
        fused = (_fusable(embeds, kept, st.video_embeds, deep) and (pos_in is None or pos_in.shape[0] <= 4))
        if fused:
            from ..fused import gather_scatter, keep_positions_batched, repad_rows
            lay = keep_positions_batched(vm, kept, int(st.video_embeds.shape[0]), pad_left,
                                         vpm if want_vis else None, am64, pos_in, text_row0,
                                         int(deep[0].shape[0]) if want_vis else None)
            kwargs["inputs_embeds"] = repad_rows(embeds, lay.keep)
            if want_vis:
                kwargs["deepstack_visual_embeds"] = gather_scatter(list(deep), lay.vis_rows, check=False)
        else:
            lay = _batched_layout(vm, kept, pad_left, am64, pos_in.to(torch.int64) if pos_in is not None else None,
                                  text_row0, vpm if want_vis else None)
            kwargs["inputs_embeds"] = _gather_slots(embeds, lay.keep, 0)
            if want_vis:
                kwargs["deepstack_visual_embeds"] = [d[lay.vis_rows.to(d.device)] for d in deep]
        keep, Sp = lay.keep, lay.S
        if torch.is_tensor(kwargs.get("input_ids")):
            kwargs["input_ids"] = _gather_slots(kwargs["input_ids"], keep.to(kwargs["input_ids"].device), 0)
        mask = lay.mask if am_dtype == torch.int64 else lay.mask.to(am_dtype)
        kwargs["attention_mask"] = mask if am is None else mask.to(am.device)
        if pos_in is not None:
            out = lay.pos.view(torch.float64) if as_bits else lay.pos
            out = out.to(pos.dtype) if torch.is_tensor(pos) else out
            kwargs["position_ids"] = out[0] if squeeze else out
        cp = kwargs.get("cache_position")
        if torch.is_tensor(cp) and cp.dim() == 1 and cp.numel() == S:
            kwargs["cache_position"] = torch.arange(Sp, device=cp.device, dtype=cp.dtype)
        if vpm is not None:
            kwargs["visual_pos_masks"] = _gather_slots(vpm, keep, False)
        st.kept_video, st.keep_token_indices, st.lengths, st.pruned = kept, keep, lay.lengths, True
        st.decode = _DecodeLayout(mask, keep, S, S - lay.lengths if self._renumber else None)


def decode_state(model, clear: bool = False) -> Optional[_DecodeLayout]:
    """The layout a batched pruned prefill left for the decode steps behind it (None: none); clear=True drops it."""
    if clear:
        return model.__dict__.pop("_vidcom2_decode", None)
    return model.__dict__.get("_vidcom2_decode")


class _DecodeShim:
    """Stands in for `self.language_model` during a decode step behind a batched pruned prefill: maps the attention
    mask generate built for the unpruned prompt onto the pruned layout of the KV cache."""

    def __init__(self, real, dec: _DecodeLayout):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_dec", dec)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_real"), name)

    def __call__(self, *args, **kwargs):
        embeds = kwargs.get("inputs_embeds")
        cache = kwargs.get("past_key_values")
        if torch.is_tensor(embeds) and cache is not None:
            past = int(cache.get_seq_length())
            kwargs["attention_mask"] = _map_decode_mask(kwargs.get("attention_mask"), self._dec, past, embeds.shape[1],
                                                        embeds.shape[0])
            dropped, pos = self._dec.dropped, kwargs.get("position_ids")
            if dropped is not None and torch.is_tensor(pos) and pos.dim() == 2 and pos.shape[0] % dropped.shape[0] == 0:
                # generate counts on from the UNPRUNED prompt's last position; the pruned one ended `dropped` earlier
                dropped = dropped.repeat_interleave(pos.shape[0] // dropped.shape[0], 0)
                kwargs["position_ids"] = pos - dropped.to(device=pos.device, dtype=pos.dtype)[:, None]
        return self._real(*args, **kwargs)


def run_decode_step(model, forward: Callable, lm_attr: str = "language_model"):
    with shadow(model, **{lm_attr: _DecodeShim(getattr(model, lm_attr), decode_state(model))}):
        return forward()


def run_with_pruning(model, forward: Callable, choose: Callable[[torch.Tensor], Optional[torch.Tensor]],
                     lm_attr: str = "language_model",
                     choose_many: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, renumber: bool = False):
    """Run `forward()` with the interceptors in place.  `choose(video_embeds)` returns the sorted
    kept indices into the video token list (or None to leave the prompt alone); `choose_many` the same for a batch of
    B > 1 prompts (None: such batches are left alone); `renumber`: positions as if the dropped tokens had never been in the
    prompt (module docstring)."""
    state = PruneState()
    mask_inner = model.get_placeholder_mask

    def get_placeholder_mask(*args, **kwargs):
        out = mask_inner(*args, **kwargs)
        feats = kwargs.get("video_features")
        if feats is not None:
            vmask = out[1]
            st_mask = vmask[..., 0] if vmask.dim() == 3 else vmask
            state.video_mask, state.video_embeds = st_mask.bool(), feats
        return out

    shim = _LanguageModelShim(getattr(model, lm_attr), state, choose, choose_many, renumber)
    with shadow(model, get_placeholder_mask=get_placeholder_mask, **{lm_attr: shim}):
        out = forward()
    model.__dict__["_vidcom2_last"] = state
    if state.decode is not None:
        model.__dict__["_vidcom2_decode"] = state.decode
    return out

"""Voice prefix cache: the K / V of the voice-only head of a prompt, computed once and restored into a KV cache per generate() call.

`VibeVoiceProcessor._process_single` builds every prompt as  system prompt | " Voice input:\\n" + the speakers' voice placeholders |
" Text input:\\n" | script lines | " Speech output:\\n" <speech_start>.  The first three parts depend on the voices alone and attention is
causal, so their K / V do too: `model.prepare_voice_prefix` runs the voice encode and the prefill of those P positions once and keeps the
result in a `VoicePrefix`; `generate(voice_prefix=...)` restores it with one `vv_kv_copy` launch and prefills only the script part at
position P.  The store is an ordinary `vv_kv` (rows = 1, s_max = ceil64(P), no vt) in the cache's compute dtype - for an fp8 KV cache the
bf16 values of the staging cache, so the scales are still derived from the whole prompt.  It is read-only after `prepare_voice_prefix`
returns (which synchronises), so any stream may read it; the model keeps no registry, the caller owns the object.

This module is host logic only (no torch.cuda call): the checks run on a machine without a GPU."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _lib as L


@dataclass
class VoicePrefix:
    ids: torch.Tensor            # [P] int64, CPU: the prefix token ids (voice placeholders included)
    P: int                       # prefix length = cache slots [0, P)
    k: torch.Tensor              # [layers][1][kv_heads][ceil64(P)][head_dim], the cache's compute dtype
    v: torch.Tensor
    kv: L.KV                     # the vv_kv describing k / v (rows = 1, vt = NULL)
    nbytes: int                  # device bytes the store holds (k + v)

    @property
    def layers(self) -> int:
        return int(self.kv.layers)

    @property
    def kv_heads(self) -> int:
        return int(self.kv.kv_heads)

    @property
    def head_dim(self) -> int:
        return int(self.kv.head_dim)

    @property
    def dtype(self) -> torch.dtype:
        return self.k.dtype


def store_shape(layers: int, kv_heads: int, head_dim: int, P: int) -> tuple:
    """k / v shape of a store of P slots (the caches' 64-slot granule)"""
    return (layers, 1, kv_heads, max(64, (int(P) + 63) // 64 * 64), head_dim)


def describe(k: torch.Tensor, v: torch.Tensor) -> L.KV:
    """the vv_kv of store tensors shaped by store_shape"""
    kv = L.KV()
    kv.k, kv.v, kv.vt = k.data_ptr(), v.data_ptr(), None
    kv.kvdt = L.VV_F32 if k.dtype == torch.float32 else L.VV_BF16
    kv.layers, kv.rows, kv.kv_heads, kv.s_max, kv.head_dim = k.shape
    return kv


def per_dialogue(voice_prefix, B: int) -> Optional[List[Optional[VoicePrefix]]]:
    """generate(voice_prefix=): one object for all dialogues of the batch, or a list with one entry per dialogue (None entries take the full
    path).  Returns the per-dialogue list, or None when no dialogue has a prefix."""
    if voice_prefix is None:
        return None
    vps = list(voice_prefix) if isinstance(voice_prefix, (list, tuple)) else [voice_prefix] * B
    if len(vps) != B:
        raise ValueError(f"voice_prefix: a list needs one entry per dialogue ({len(vps)} entries, {B} dialogues)")
    for vp in vps:
        if vp is not None and not isinstance(vp, VoicePrefix):
            raise ValueError(f"voice_prefix: entries are VoicePrefix objects or None, not {type(vp).__name__}")
    return vps if any(vp is not None for vp in vps) else None


def check(vp: VoicePrefix, ids: torch.Tensor, sp_mask: Optional[torch.Tensor], layers: int, kv_heads: int, head_dim: int, dtype: torch.dtype,
          where: str = "") -> None:
    """A dialogue's prompt (left padding stripped) against the prefix it is to start from: ValueError naming what differs - never a silent full
    prefill, and never another voice's K / V under this prompt."""
    P = vp.P
    got = (vp.layers, vp.kv_heads, vp.head_dim, vp.dtype)
    if got != (layers, kv_heads, head_dim, dtype):
        raise ValueError(f"voice_prefix{where}: the store was prepared by a model with other shapes: (layers, kv_heads, head_dim, dtype) = {got}, "
                         f"this model has {(layers, kv_heads, head_dim, dtype)}")
    ids = torch.as_tensor(ids).reshape(-1).cpu()
    if ids.numel() <= P:
        raise ValueError(f"voice_prefix{where}: the prompt has {ids.numel()} tokens and the prefix {P}: the prompt must be longer than the prefix")
    diff = (ids[:P] != vp.ids).nonzero()
    if diff.numel():
        i = int(diff[0])
        raise ValueError(f"voice_prefix{where}: the prompt does not start with the prefix ids: {int(diff.shape[0])} of {P} positions differ, the first at "
                         f"{i} (prompt {int(ids[i])}, prefix {int(vp.ids[i])})")
    if sp_mask is not None:
        late = torch.as_tensor(sp_mask).reshape(-1).bool()[P:].nonzero()
        if late.numel():
            raise ValueError(f"voice_prefix{where}: speech_input_mask marks position {P + int(late[0])}, at or beyond the prefix length {P}: every voice "
                             "placeholder must lie inside the prefix")

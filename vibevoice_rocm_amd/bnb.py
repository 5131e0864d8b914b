"""Pre-quantized bitsandbytes 4-bit NF4 checkpoints (what `save_pretrained` writes for a model loaded with BitsAndBytesConfig(load_in_4bit=True,
bnb_4bit_quant_type="nf4")), restated from bitsandbytes' functional.quantize_4bit / dequantize_4bit and QuantState.as_dict(packed=True) / from_dict.

For each quantised nn.Linear X the safetensors shards hold
  X.weight                                  uint8, ceil(N*K/2) bytes over the row-major FLATTENED [N, K] weight: element 2i is the high nibble of
                                            byte i, element 2i+1 the low nibble
  X.weight.quant_state.bitsandbytes__nf4    uint8 bytes of a UTF-8 JSON object: quant_type, blocksize, dtype, shape [N, K]; with double
                                            quantisation also nested_blocksize, nested_dtype, nested_offset
  X.weight.quant_map                        fp32 [16], the NF4 code book
  X.weight.absmax                           fp32 [nblocks] (uint8 [nblocks] with double quantisation); nblocks = ceil(N*K / blocksize), the blocks
                                            run over the flattened weight and straddle rows when K % blocksize != 0
  X.weight.nested_absmax                    double quantisation: fp32 [ceil(nblocks / nested_blocksize)]
  X.weight.nested_quant_map                 double quantisation: fp32 [256], bnb's dynamic map (used as stored)
Decoded, in fp32 with every operation rounded on its own:
  absmax[b] = (nested_quant_map[absmax_u8[b]] * nested_absmax[b // nested_blocksize]) + nested_offset   (or the stored fp32 value)
  w[j]      = bf16_rne(quant_map[code_j] * absmax[j // blocksize])                                     (the VV_NF4 definition, bf16 compute)
`vv_nf4_import` (include/vv_hip.h) is the device form; `dequantize` here is the host restatement the tests hold it to.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .weights import NF4_BLOCK, NF4_TABLE

QS_PREFIX = ".quant_state.bitsandbytes__"
COMPANION_SUFFIXES = ("absmax", "quant_map", "nested_absmax", "nested_quant_map")


@dataclass
class BnbNF4:
    """One quantised matrix as the checkpoint holds it (host or device tensors) and its parsed quant state."""
    name: str                       # the weight's state-dict key, e.g. "model.language_model.layers.0.mlp.up_proj.weight"
    shape: Tuple[int, ...]
    blocksize: int
    dtype: str                      # bnb's compute dtype name ("float16", "bfloat16", ...); served as bf16 whatever it says
    weight: torch.Tensor            # uint8 [ceil(numel / 2)]
    absmax: torch.Tensor            # fp32 [nblocks], or uint8 [nblocks] when nested
    quant_map: torch.Tensor         # fp32 [16]
    nested_absmax: Optional[torch.Tensor] = None
    nested_quant_map: Optional[torch.Tensor] = None
    nested_blocksize: int = 0
    nested_offset: float = 0.0

    @property
    def n(self) -> int:
        return int(self.shape[0])

    @property
    def k(self) -> int:
        return self.numel // self.n

    @property
    def numel(self) -> int:
        p = 1
        for s in self.shape:
            p *= int(s)
        return p

    @property
    def nblocks(self) -> int:
        return -(-self.numel // self.blocksize)

    @property
    def nested(self) -> bool:
        return self.nested_absmax is not None

    def companion_exact(self) -> bool:
        """Whether the VV_NF4 companion can hold this matrix's codes and scales exactly: 64-blocks that never cross a row."""
        return self.k % NF4_BLOCK == 0 and self.blocksize % NF4_BLOCK == 0 and self.k % self.blocksize == 0

    def to(self, device) -> "BnbNF4":
        mv = lambda t: None if t is None else t.to(device).contiguous()     # noqa: E731
        return BnbNF4(self.name, self.shape, self.blocksize, self.dtype, mv(self.weight), mv(self.absmax), mv(self.quant_map),
                      mv(self.nested_absmax), mv(self.nested_quant_map), self.nested_blocksize, self.nested_offset)


def parse_quant_state(t: torch.Tensor) -> dict:
    """The JSON object bnb packs into X.weight.quant_state.bitsandbytes__<type> (uint8 bytes of UTF-8 text)."""
    if t.dtype != torch.uint8:
        raise ValueError(f"a bitsandbytes quant_state must be uint8 bytes, got {t.dtype}")
    return json.loads(bytes(t.detach().cpu().reshape(-1).tolist()).decode("utf-8"))


def split_prequantized(sd: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], Dict[str, BnbNF4]]:
    """(plain tensors, {weight key: BnbNF4}) of a loaded checkpoint.  Follows what the file holds: a weight with a quant_state sibling is a
    bnb matrix, every other tensor is plain.  Refuses fp4, a code book other than NF4's, non-uint8 storage and missing or stray companion keys."""
    qs_keys = [k for k in sd if QS_PREFIX in k]
    records: Dict[str, BnbNF4] = {}
    used = set()
    for qk in qs_keys:
        name, qtype = qk.split(QS_PREFIX)
        state = parse_quant_state(sd[qk])
        qt = str(state.get("quant_type", qtype)).lower()
        if qt == "fp4" or qtype == "fp4":
            raise NotImplementedError(f"{name}: bitsandbytes fp4 checkpoints are not built (only nf4)")
        if qt != "nf4" or qtype != "nf4":
            raise ValueError(f"{name}: unknown bitsandbytes quant_type {qt!r} / {qtype!r}")
        nested = "nested_blocksize" in state or (name + ".nested_absmax") in sd
        need = [name, name + ".absmax", name + ".quant_map"] + ([name + ".nested_absmax", name + ".nested_quant_map"] if nested else [])
        missing = [k for k in need if k not in sd]
        if missing:
            raise ValueError(f"{name}: bitsandbytes NF4 matrix is missing {missing}")
        for f in ("blocksize", "shape") + (("nested_blocksize", "nested_offset") if nested else ()):
            if f not in state:
                raise ValueError(f"{name}: quant_state has no {f!r}")
        w = sd[name]
        if w.dtype != torch.uint8:
            raise ValueError(f"{name}: quant_storage {w.dtype} is not built (bitsandbytes' default uint8 only)")
        qm = sd[name + ".quant_map"]
        if qm.dtype != torch.float32 or not torch.equal(qm.reshape(-1).cpu(), torch.tensor(NF4_TABLE, dtype=torch.float32)):
            raise ValueError(f"{name}: quant_map is not the NF4 code book")
        rec = BnbNF4(name=name, shape=tuple(int(s) for s in state["shape"]), blocksize=int(state["blocksize"]), dtype=str(state.get("dtype", "")),
                     weight=w.reshape(-1), absmax=sd[name + ".absmax"].reshape(-1), quant_map=qm.reshape(-1),
                     nested_absmax=sd[name + ".nested_absmax"].reshape(-1) if nested else None,
                     nested_quant_map=sd[name + ".nested_quant_map"].reshape(-1) if nested else None,
                     nested_blocksize=int(state["nested_blocksize"]) if nested else 0,
                     nested_offset=float(state["nested_offset"]) if nested else 0.0)
        _check_sizes(rec)
        records[name] = rec
        used.update(need + [qk])
    stray = [k for k in sd if k not in used and any(k.endswith(".weight." + s) for s in COMPANION_SUFFIXES)]
    if stray:
        raise ValueError(f"bitsandbytes tensors without a quant_state: {stray[:4]}")
    plain = {k: v for k, v in sd.items() if k not in used}
    return plain, records


def _check_sizes(r: BnbNF4) -> None:
    if len(r.shape) < 2 or r.numel <= 0 or r.blocksize <= 0:
        raise ValueError(f"{r.name}: bad quant_state shape {r.shape} / blocksize {r.blocksize}")
    if r.weight.numel() != -(-r.numel // 2):
        raise ValueError(f"{r.name}: {r.weight.numel()} packed bytes for shape {r.shape} (want {-(-r.numel // 2)})")
    want_dt = torch.uint8 if r.nested else torch.float32
    if r.absmax.dtype != want_dt or r.absmax.numel() != r.nblocks:
        raise ValueError(f"{r.name}: absmax {r.absmax.dtype} [{r.absmax.numel()}], want {want_dt} [{r.nblocks}]")
    if r.nested:
        if r.nested_blocksize <= 0:
            raise ValueError(f"{r.name}: nested_blocksize {r.nested_blocksize}")
        nn = -(-r.nblocks // r.nested_blocksize)
        if r.nested_absmax.dtype != torch.float32 or r.nested_absmax.numel() != nn:
            raise ValueError(f"{r.name}: nested_absmax {r.nested_absmax.dtype} [{r.nested_absmax.numel()}], want float32 [{nn}]")
        if r.nested_quant_map.dtype != torch.float32 or r.nested_quant_map.numel() != 256:
            raise ValueError(f"{r.name}: nested_quant_map must be float32 [256]")


def check_shapes(records: Dict[str, BnbNF4], shapes: Dict[str, Sequence[int]]) -> None:
    """Every bnb matrix must be a tensor of the model with the model's shape (quant_state's `shape` against the config)."""
    for name, r in records.items():
        if name not in shapes:
            raise ValueError(f"{name}: bitsandbytes matrix that the model does not have")
        if tuple(r.shape) != tuple(shapes[name]):
            raise ValueError(f"{name}: quant_state shape {list(r.shape)} disagrees with the config's {list(shapes[name])}")


# ---- host restatement ------------------------------------------------------------------------------------------------
def block_absmax(r: BnbNF4) -> torch.Tensor:
    """fp32 [nblocks]: the stored scales, or the double-quantised ones decoded ((map[code] * nested_absmax) + offset, two roundings)."""
    if not r.nested:
        return r.absmax.float()
    idx = torch.arange(r.nblocks, device=r.absmax.device) // r.nested_blocksize
    v = r.nested_quant_map.float()[r.absmax.long()] * r.nested_absmax.float()[idx]
    return v + torch.tensor(r.nested_offset, dtype=torch.float32, device=v.device)


def codes(r: BnbNF4) -> torch.Tensor:
    """uint8 [numel]: the 4-bit code of every flattened element (high nibble first)."""
    b = r.weight
    return torch.stack([b >> 4, b & 15], dim=1).reshape(-1)[: r.numel].contiguous()


def dequantize(r: BnbNF4) -> torch.Tensor:
    """fp32 [N, K]: bf16_rne(quant_map[code] * absmax[j // blocksize]), every value exact in bf16."""
    am = block_absmax(r)
    j = torch.arange(r.numel, device=am.device)
    v = r.quant_map.float()[codes(r).long()] * am[j // r.blocksize]
    return v.to(torch.bfloat16).float().reshape(r.n, r.k)


def effective_state_dict(plain: Dict[str, torch.Tensor], records: Dict[str, BnbNF4]) -> Dict[str, torch.Tensor]:
    """The state dict an engine loaded from this checkpoint computes with (the checker side of parity tests): plain tensors as they are,
    bnb matrices dequantised (fp32, in their quant_state shape)."""
    out = dict(plain)
    for name, r in records.items():
        out[name] = dequantize(r).reshape(r.shape)
    return out


# ---- device import ---------------------------------------------------------------------------------------------------
def import_nf4(parts: List[BnbNF4], device, companion: bool):
    """vv_nf4_import of one or more bnb matrices stacked along N (q, k, v -> the fused [q|k|v]): returns (bf16 [sum N, K] row-major, VV_NF4
    codes, VV_NF4 scales) - the last two None unless `companion` (every part must then satisfy companion_exact).  Enqueued on the current stream,
    which the temporaries' device copies belong to."""
    from . import _lib as L
    lib = L.load()
    device = torch.device(device)
    k = parts[0].k
    if any(p.k != k for p in parts):
        raise ValueError("stacked bnb matrices must share K")
    rows = sum(p.n for p in parts)
    w = torch.empty(rows, k, dtype=torch.bfloat16, device=device)
    cq = cs = None
    if companion:
        nq, ku = (rows + 3) // 4, (k + 511) // 512
        cq = torch.zeros(nq * ku * 1024, dtype=torch.uint8, device=device)
        cs = torch.zeros(nq * ku * 32, dtype=torch.float32, device=device)
    sp = torch.cuda.current_stream(device).cuda_stream
    row0 = 0
    for p in parts:
        d = p.to(device)
        s = L.Nf4Src()
        s.packed, s.absmax, s.quant_map = d.weight.data_ptr(), d.absmax.data_ptr(), d.quant_map.data_ptr()
        s.nested_absmax = d.nested_absmax.data_ptr() if d.nested else None
        s.nested_map = d.nested_quant_map.data_ptr() if d.nested else None
        s.nested_offset, s.nested_blocksize = d.nested_offset, d.nested_blocksize
        s.n, s.k, s.blocksize = d.n, d.k, d.blocksize
        L.check(lib.vv_nf4_import(C.byref(s), w.data_ptr(), k, row0, rows, L.ptr(cq), L.ptr(cs), sp), f"vv_nf4_import {p.name}")
        row0 += p.n
    return w, cq, cs

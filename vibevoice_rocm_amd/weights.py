"""Device-resident weights in the layout the MI355X kernels stream, plus the ctypes descriptors that point at them.

Input is a flat state dict with the reference's tensor names (`synth.state_dict_shapes`).
Re-layouts done once at load time (HBM is 288 GB: we spend bytes to make every per-frame read a straight stream):
  * q/k/v projection rows concatenated into one [q+2kv, H] matrix (+ one bias vector) -> one GEMV per layer;
  * dense SConv1d weights [C_out, C_in, k] -> [C_out, k*C_in] (tap-major) so a conv is a GEMM over the
    channels-last activation buffer read in place with overlapping rows;
  * SConvTranspose1d weights [C_in, C_out, 2s] -> [(r, C_out), (j, C_in)] (j = 0 previous input, 1 current), bias
    tiled over r: a transposed conv with k = 2s is one GEMM producing s output rows per input row;
  * depthwise taps [C, 1, 7] -> [C, 7] fp32; every 1-D tensor fp32.
Matrix weights are stored in `wdtype` (fp32 for graded parity, bf16 for the benchmark configs).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from . import _lib as L
from .config import VVConfig


def _wdt(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return L.VV_F32
    if dtype == torch.bfloat16:
        return L.VV_BF16
    raise ValueError(f"unsupported weight dtype {dtype}")


FP8_MAX = 448.0      # largest finite e4m3fn magnitude


def quantize_e4m3_pow2(w: torch.Tensor):
    """Weight-only fp8 of a [N, K] matrix: one POWER-OF-TWO scale per output row (2^ceil(log2(amax / 448))) and round-to-nearest
    e4m3fn codes.  With a power-of-two scale the dequantised weight code * scale is exactly representable in bf16, so the bf16
    copy the GEMM-shaped uses keep (prefill, T > 4) and the fp8 copy the decode GEMVs stream are the SAME effective matrix.
    Returns (codes uint8 [N, K], scale fp32 [N], effective weights fp32 [N, K])."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1).clamp_min(1e-30)
    scale = torch.exp2(torch.ceil(torch.log2(amax / FP8_MAX)))
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), scale.contiguous(), q.float() * scale[:, None]


def fp8_matrix_names(cfg: VVConfig):
    """State-dict keys of the matrices that run as weight-streaming GEMVs every frame and get an fp8 companion: the LLM's linears,
    the diffusion head's SwiGLU matrices, the FFN linears of the 1-row conv stage (decoder stage 0 / semantic-encoder last stage)."""
    names = []
    for l in range(cfg.layers):
        q = f"model.language_model.layers.{l}."
        names += [q + f"self_attn.{n}_proj.weight" for n in "qkvo"] + [q + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    for l in range(cfg.head_layers):
        q = f"model.prediction_head.layers.{l}."
        names += [q + f"ffn.{n}_proj.weight" for n in ("gate", "up", "down")]
    n_st = len(cfg.ac_ratios) + 1
    for j in range(cfg.ac_depths[-1]):
        names += [f"model.acoustic_tokenizer.decoder.stages.0.{j}.ffn.linear{i}.weight" for i in (1, 2)]
    for j in range(cfg.sem_depths[-1]):
        names += [f"model.semantic_tokenizer.encoder.stages.{n_st - 1}.{j}.ffn.linear{i}.weight" for i in (1, 2)]
    return names


# bitsandbytes' NF4 code book (index = 4-bit code), in this order
NF4_TABLE = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
             -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
             0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
NF4_BLOCK = 64


def _nf4_thresholds() -> torch.Tensor:
    """The 15 decision thresholds of bnb's dQuantizeNF4: midpoints of neighbouring table entries (fp64 midpoint, fp32 constant)."""
    t = torch.tensor(NF4_TABLE, dtype=torch.float64)
    return ((t[1:] + t[:-1]) / 2).float()


def quantize_nf4(w: torch.Tensor):
    """Weight-only blockwise NF4 of a [N, K] matrix (K % 64 == 0), bitsandbytes' definition restated:
      * blocks are 64 consecutive weights along K within an output row;
      * absmax = fp32 max |w| over the block (w = the weight widened to fp32);
      * code = index of the table entry nearest to w * (1 / absmax) (fp32), ties to the lower code (bnb compares x > midpoint);
      * a block with absmax == 0 gets code 7 (0.0) and scale 0;
      * effective weight = bf16_rne(fp32(table[code]) * absmax): bnb's dequantisation with bf16 as compute dtype (there is no fp16 path).
    Double quantisation of the scales is not reproduced: absmax stays fp32.
    Returns (codes uint8 [N, K], absmax fp32 [N, K / 64], effective weights fp32 [N, K], every value exactly bf16-representable)."""
    n, k = w.shape
    if k % NF4_BLOCK:
        raise ValueError(f"NF4 needs K % {NF4_BLOCK} == 0 (K={k})")
    wf = w.detach().float().reshape(n, k // NF4_BLOCK, NF4_BLOCK)
    absmax = wf.abs().amax(dim=2)
    zero = absmax == 0
    inv = torch.where(zero, torch.zeros_like(absmax), torch.reciprocal(absmax))
    x = (wf * inv[..., None]).contiguous()
    codes = torch.searchsorted(_nf4_thresholds().to(x.device), x, right=False).to(torch.uint8)   # number of thresholds t with x > t
    codes = torch.where(zero[..., None], torch.full_like(codes, 7), codes)
    table = torch.tensor(NF4_TABLE, dtype=torch.float32, device=x.device)
    eff = (table[codes.long()] * absmax[..., None]).to(torch.bfloat16).float()
    return codes.reshape(n, k).contiguous(), absmax.contiguous(), eff.reshape(n, k).contiguous()


def _pack_nibbles(codes: torch.Tensor) -> torch.Tensor:
    """4-bit codes uint8 [N, K] -> the streaming GEMV's code layout (VV_NF4 and VV_MXFP4 share it, include/vv_hip.h), padded with code 0:
    [ceil(N/4)][ceil(K/512)][64 lanes][4 rows][4 B] - nibble i of dword r of lane l's 16 bytes is code (4 q + r, 512 u + 8 l + i).  uint8 1-D."""
    n, k = codes.shape
    nq, ku = (n + 3) // 4, (k + 511) // 512
    c = torch.zeros(nq * 4, ku * 512, dtype=torch.uint8, device=codes.device)
    c[:n, :k] = codes
    c = c.view(nq, 4, ku, 64, 4, 2).permute(0, 2, 3, 1, 4, 5)           # [q, u, lane, r, byte, nibble]
    return (c[..., 0] | (c[..., 1] << 4)).contiguous().view(-1)


def _unpack_nibbles(packed: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """Inverse of _pack_nibbles: codes uint8 [N, K]."""
    nq, ku = (n + 3) // 4, (k + 511) // 512
    b = packed.view(nq, ku, 64, 4, 4)
    c = torch.stack([b & 15, b >> 4], dim=-1)                           # [q, u, lane, r, byte, nibble]
    return c.permute(0, 3, 1, 2, 4, 5).reshape(nq * 4, ku * 512)[:n, :k].contiguous()


def pack_nf4(codes: torch.Tensor, absmax: torch.Tensor):
    """(codes uint8 [N, K], absmax fp32 [N, K / 64]) -> the streaming GEMV's VV_NF4 layout (include/vv_hip.h), padded with code 0 / scale 0:
    the codes as _pack_nibbles lays them out and absmax [ceil(N/4)][ceil(K/512)][4 rows][8 blocks].  Returns (uint8 1-D, fp32 1-D)."""
    n, k = codes.shape
    nq, ku = (n + 3) // 4, (k + 511) // 512
    s = torch.zeros(nq * 4, ku * 8, dtype=torch.float32, device=absmax.device)
    s[:n, : k // NF4_BLOCK] = absmax
    return _pack_nibbles(codes), s.view(nq, 4, ku, 8).permute(0, 2, 1, 3).contiguous().view(-1)


def unpack_nf4(packed: torch.Tensor, scales: torch.Tensor, n: int, k: int):
    """Inverse of pack_nf4: (codes uint8 [N, K], absmax fp32 [N, K / 64])."""
    nq, ku = (n + 3) // 4, (k + 511) // 512
    return _unpack_nibbles(packed, n, k), scales.view(nq, ku, 4, 8).permute(0, 2, 1, 3).reshape(nq * 4, ku * 8)[:n, : k // NF4_BLOCK].contiguous()


# OCP Microscaling (MX v1.0) FP4: e2m1 element values by code (codes 8..15 are the negated values), 32-element blocks with one E8M0 scale byte
MXFP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MXFP4_BLOCK = 32
# the E8M0 scale bytes the engine writes, for every MX format; 127 = 2^0 (padding, all-zero blocks)
MXFP4_SCALE_MIN, MXFP4_SCALE_MAX, MXFP4_SCALE_ONE = MXFP6_SCALE_MIN, MXFP6_SCALE_MAX, MXFP6_SCALE_ONE = 2, 252, 127
# limits of the MX rows kernel's decision (csrc/vv_gemv_rows.hip, vv_gemv_rows_decide) that the host acts on: the adaLN-modulated prologue
# is served on whole rows only (K <= 2048); the SwiGLU pair splits K two ways at most inside the row-batched step's partials workspace
# (csrc/vv_model.hip, rows_part_floats), 2 slices x 8 waves x 2 loads x 128 = 4096
MXFP4_ROWS_MOD_K, MXFP4_ROWS_MAX_HIDDEN = 2048, 4096
# MXFP6 rows (csrc/vv_gemv_rows_mx6.hip): the same decision with the same 128-wide loads, so the same two limits
MXFP6_ROWS_MOD_K, MXFP6_ROWS_MAX_HIDDEN = MXFP4_ROWS_MOD_K, MXFP4_ROWS_MAX_HIDDEN


def _quantize_mx(w: torch.Tensor, values, block: int, sign_code: int):
    """What quantize_mxfp4 / quantize_mxfp6 define, for an e2mX grid `values` (magnitudes by code; sign_code: the negative zero's code, a code's
    top bit).  The grid's spacing is values[1] below 2 (subnormals and the first binade) and doubles per binade up to the largest value's."""
    n, k = w.shape
    if k % block:
        raise ValueError(f"MXFP{sign_code.bit_length()} needs K % {block} == 0 (K={k})")
    top, emax = values[-1], math.frexp(values[-1])[1] - 1                        # emax: the exponent of the largest value, 2 for e2m1 and e2m3
    wf = w.detach().float().reshape(n, k // block, block)
    amax = wf.abs().amax(dim=2)
    zero = amax == 0
    ex = torch.frexp(torch.where(zero, torch.ones_like(amax), amax))[1] - 1      # floor(log2(amax)), exact: amax = m 2^ex', m in [0.5, 1)
    e = torch.where(zero, torch.full_like(ex, MXFP4_SCALE_ONE), (ex - emax + 127).clamp(MXFP4_SCALE_MIN, MXFP4_SCALE_MAX))
    # w / 2^(e - 127) in fp64: the quotient by a power of two is exact there for every fp32 w and every scale byte
    x = wf.double() * torch.exp2((127 - e).double())[..., None]
    a = x.abs()
    # round to nearest even on the grid (torch.round is half-to-even; a quotient by the power-of-two spacing is exact); above the top saturates
    step = values[1] * torch.exp2((torch.frexp(a)[1] - 1).clamp(0, emax).double())
    q = (torch.round(a / step) * step).clamp_max(top)
    grid = torch.tensor(values, dtype=torch.float64, device=q.device)
    mag = torch.searchsorted(grid, q.contiguous()).to(torch.uint8)               # q is on the grid: its index
    codes = torch.where((x < 0) & (mag > 0), mag + sign_code, mag).to(torch.uint8)
    eff = (torch.where(x < 0, -q, q) * torch.exp2((e - 127).double())[..., None]).float()
    eff = torch.where(mag == 0, torch.zeros_like(eff), eff)                      # +0, as code 0 decodes
    return codes.reshape(n, k).contiguous(), e.to(torch.uint8).contiguous(), eff.reshape(n, k).contiguous()


def quantize_mxfp4(w: torch.Tensor):
    """Weight-only MXFP4 of a [N, K] matrix (K % 32 == 0), the OCP MX v1.0 conversion:
      * blocks are 32 consecutive weights along K within an output row;
      * scale byte e = clamp(floor(log2(max |w|)) - 2 + 127, 2, 252), worth 2^(e - 127) (2 = the exponent of e2m1's largest value 6); an
        all-zero block gets 127;
      * element = w / scale rounded to nearest, ties to even, on the e2m1 grid {0, 0.5, 1, 1.5, 2, 3, 4, 6}, saturating at +-6; a value that
        rounds to zero takes code 0 (never the negative zero, code 8);
      * effective weight = value(code) * 2^(e - 127): exact in bf16 (and so in fp32).
    Returns (codes uint8 [N, K], scale bytes uint8 [N, K / 32], effective weights fp32 [N, K])."""
    return _quantize_mx(w, MXFP4_VALUES, MXFP4_BLOCK, 8)


def pack_mxfp4(codes: torch.Tensor, scales: torch.Tensor):
    """(codes uint8 [N, K], scale bytes uint8 [N, K / 32]) -> the VV_MXFP4 layout (include/vv_hip.h), padded with code 0 / scale byte 127:
    the codes as _pack_nibbles lays them out and scale bytes [ceil(N/4)][ceil(K/512)][16 blocks][4 rows].  Returns (uint8 1-D, uint8 1-D)."""
    n, k = codes.shape
    nq, ku = (n + 3) // 4, (k + 511) // 512
    s = torch.full((nq * 4, ku * 16), MXFP4_SCALE_ONE, dtype=torch.uint8, device=scales.device)
    s[:n, : k // MXFP4_BLOCK] = scales
    return _pack_nibbles(codes), s.view(nq, 4, ku, 16).permute(0, 2, 3, 1).contiguous().view(-1)  # [q, u, block, r]


def unpack_mxfp4(packed: torch.Tensor, sb: torch.Tensor, n: int, k: int):
    """Inverse of pack_mxfp4: (codes uint8 [N, K], scale bytes uint8 [N, K / 32])."""
    nq, ku = (n + 3) // 4, (k + 511) // 512
    return _unpack_nibbles(packed, n, k), sb.view(nq, ku, 16, 4).permute(0, 3, 1, 2).reshape(nq * 4, ku * 16)[:n, : k // MXFP4_BLOCK].contiguous()


# OCP Microscaling (MX v1.0) FP6, the e2m3 variant: 1 sign, 2 exponent, 3 mantissa bits (codes 0..31 below, 32..63 the same values negated) -
# subnormals m / 8 for m = 0..7, normals (1 + m / 8) * 2^(E - 1) for E = 1..3, the largest 7.5; 32-element blocks with one E8M0 scale byte
MXFP6_VALUES = tuple(m / 8.0 for m in range(8)) + tuple((1.0 + m / 8.0) * 2.0 ** (E - 1) for E in (1, 2, 3) for m in range(8))
MXFP6_BLOCK = 32
# Element i of a block sits in bits 6 i .. 6 i + 5 of the 192-bit operand of v_cvt_scalef32_pk32_*_fp6, counted from bit 0 of the first dword
# (tests/test_hip_mxfp6.py::test_decode_is_exact is the witness: the hardware reads every code back from there)


def quantize_mxfp6(w: torch.Tensor):
    """Weight-only MXFP6 (e2m3) of a [N, K] matrix (K % 32 == 0), the OCP MX v1.0 conversion:
      * blocks are 32 consecutive weights along K within an output row;
      * scale byte e = clamp(floor(log2(max |w|)) - 2 + 127, 2, 252), worth 2^(e - 127) (2 = the exponent of e2m3's largest value 7.5 =
        1.875 * 2^2); an all-zero block gets 127;
      * element = w / scale rounded to nearest, ties to even, on the e2m3 grid (spacing 1/8 below 2, 1/4 below 4, 1/2 up to 7.5), saturating at
        +-7.5; a value that rounds to zero takes code 0 (never the negative zero, code 32);
      * effective weight = value(code) * 2^(e - 127): four significant bits times a power of two, exact in bf16 (and so in fp32).
    Returns (codes uint8 [N, K] in 0..63, scale bytes uint8 [N, K / 32], effective weights fp32 [N, K])."""
    return _quantize_mx(w, MXFP6_VALUES, MXFP6_BLOCK, 32)


def pack_mxfp6(codes: torch.Tensor, scales: torch.Tensor):
    """(codes uint8 [N, K], scale bytes uint8 [N, K / 32]) -> the VV_MXFP6 layout (include/vv_hip.h); rows past N hold code 0 / scale byte 127
    (K is never padded: K % 32 == 0).  With G = ceil(N / 4) row groups and B = K / 32 blocks per row, a block's 24 bytes (element i in bits
    6 i .. 6 i + 5) are split into a 16-byte and an 8-byte plane: codes [G][ plane A [4 rows][B][16 B] | plane B [4 rows][B][8 B] ],
    scale bytes [G][B][4 rows].  Returns (uint8 1-D, uint8 1-D)."""
    n, k = codes.shape
    nq, nb = (n + 3) // 4, k // MXFP6_BLOCK
    c = torch.zeros(nq * 4, k, dtype=torch.uint8, device=codes.device)
    c[:n] = codes
    bits = (c.view(nq, 4, nb, 32, 1) >> torch.arange(6, device=c.device, dtype=torch.uint8)) & 1          # [q, r, b, element, bit]: the 192-bit string
    by = (bits.reshape(nq, 4, nb, 24, 8) << torch.arange(8, device=c.device, dtype=torch.uint8)).sum(dim=-1, dtype=torch.uint8)   # 24 bytes per block
    packed = torch.cat([by[..., :16].reshape(nq, -1), by[..., 16:].reshape(nq, -1)], dim=1).contiguous().view(-1)
    s = torch.full((nq * 4, nb), MXFP6_SCALE_ONE, dtype=torch.uint8, device=scales.device)
    s[:n] = scales
    sb = s.view(nq, 4, nb).permute(0, 2, 1).contiguous().view(-1)          # [q, block, r]
    return packed, sb


def unpack_mxfp6(packed: torch.Tensor, sb: torch.Tensor, n: int, k: int):
    """Inverse of pack_mxfp6: (codes uint8 [N, K], scale bytes uint8 [N, K / 32])."""
    nq, nb = (n + 3) // 4, k // MXFP6_BLOCK
    p = packed.view(nq, 4 * nb * 24)
    by = torch.cat([p[:, : 4 * nb * 16].reshape(nq, 4, nb, 16), p[:, 4 * nb * 16:].reshape(nq, 4, nb, 8)], dim=-1)          # [q, r, b, 24 bytes]
    bits = ((by[..., None] >> torch.arange(8, device=by.device, dtype=torch.uint8)) & 1).reshape(nq, 4, nb, 32, 6)
    codes = (bits << torch.arange(6, device=by.device, dtype=torch.uint8)).sum(dim=-1, dtype=torch.uint8).reshape(nq * 4, k)[:n].contiguous()
    scales = sb.view(nq, nb, 4).permute(0, 2, 1).reshape(nq * 4, nb)[:n].contiguous()
    return codes, scales


class WeightFormat(NamedTuple):
    block: Optional[int]       # weights per scale along K (a matrix whose K it does not divide gets no companion); None: fp8's one scale per output
    quantize: Callable         # row, the one format that quantises the matrix as given - the blockwise ones quantise its bf16 rounding
    pack: Optional[Callable]   # (codes, scales) -> the companion's layout (include/vv_hip.h); None: the codes are streamed as quantize gives them
    wq: int                    # the VV_WQ_* bit of the descriptors' wdt
    what: str


# weight_quant -> its format: the one place on this side that lists them (csrc/vv_kernels.hip has the kernels' table)
WEIGHT_FORMATS: Dict[str, WeightFormat] = {
    "fp8": WeightFormat(None, quantize_e4m3_pow2, None, 0, "weight-only e4m3"),
    "nf4": WeightFormat(NF4_BLOCK, quantize_nf4, pack_nf4, L.VV_WQ_NF4, "weight-only 4-bit NF4"),
    "mxfp4": WeightFormat(MXFP4_BLOCK, quantize_mxfp4, pack_mxfp4, L.VV_WQ_MXFP4, "weight-only OCP MXFP4"),
    "mxfp6": WeightFormat(MXFP6_BLOCK, quantize_mxfp6, pack_mxfp6, L.VV_WQ_MXFP6, "weight-only OCP MXFP6 e2m3"),
}


def effective_state_dict(cfg: VVConfig, sd: Dict[str, torch.Tensor], quant: str) -> Dict[str, torch.Tensor]:
    """The state dict a weight_quant=quant engine computes with (the checker side of parity tests): every matrix of fp8_matrix_names that the
    format takes replaced by its effective weights (fp32 tensors; q/k/v quantise the same fused or apart: the scales lie inside rows).  A
    matrix whose K the format's block does not divide is left as it is."""
    f = WEIGHT_FORMATS[quant]
    out = dict(sd)
    for name in fp8_matrix_names(cfg):
        if not (f.block and sd[name].shape[1] % f.block):
            out[name] = f.quantize(sd[name] if f.block is None else sd[name].to(torch.bfloat16))[2]
    return out


fp8_effective_state_dict = functools.partial(effective_state_dict, quant="fp8")       # (cfg, sd) -> state dict, one per format as ever
nf4_effective_state_dict = functools.partial(effective_state_dict, quant="nf4")
mxfp4_effective_state_dict = functools.partial(effective_state_dict, quant="mxfp4")
mxfp6_effective_state_dict = functools.partial(effective_state_dict, quant="mxfp6")


class DeviceWeights:
    """Owns every device tensor of the model and the C descriptors (vv_llm, vv_head, vv_convnet x3, vv_connector x2)."""

    def __init__(self, cfg: VVConfig, sd: Dict[str, torch.Tensor], device, wdtype=torch.bfloat16, streaming_state=True, quant=None,
                 prequant: Optional[Dict[str, object]] = None, mxfp4_row_batch: bool = False, mxfp4_lean: bool = False,
                 mxfp6_row_batch: bool = False, mxfp6_lean: bool = False):
        """prequant: the matrices a pre-quantized bitsandbytes NF4 checkpoint holds in 4-bit form ({weight key: bnb.BnbNF4}, not in `sd`); they
        are imported as they are (vv_nf4_import) and need quant="nf4".  mxfp4_row_batch (quant="mxfp4" only): the 3..8-row paths stream the
        MXFP4 companions in fragment-major form (VV_WQ_FRAG4 on the LLM's and the head's descriptors; ensure_frag builds the copies).
        mxfp6_row_batch (quant="mxfp6" only): the same for the MXFP6 companions (VV_WQ_FRAG6, the VV_MXFP6_FRAG form); the bf16 matrices stay unless mxfp6_lean drops the LLM's.
        mxfp4_lean (quant="mxfp4" only): the LLM's matrices exist as MXFP4 codes alone - no bf16 copy is uploaded, their descriptor pointers are
        NULL and every pass of 3 or more prompt rows runs the GEMM on the codes (csrc/vv_gemm_mx.hip; lean_report lists what was dropped).
        mxfp6_lean (quant="mxfp6" only): the same for the MXFP6 codes (csrc/vv_gemm_mx6.hip), with the same list of what is kept.
        Kept in bf16, because something still reads them in that form:
          * matrices without a companion (embeddings / lm_head, the head's projections and adaLN, connectors, the tokenizers' convs);
          * a companion-set matrix whose shape the GEMM refuses (N % 16, K % 128) - then none of the LLM's is dropped, a model is lean as a whole;
          * the diffusion head's gate / up / down: vv_head_forward and the row-batched samplers read them row-major at more than two rows (with
            mxfp4_row_batch the pair at K > MXFP4_ROWS_MOD_K has no fragment copy and runs on the bf16 matrix, ensure_frag);
          * the tokenizers' one-row-stage FFN matrices: the same blocks run as GEMMs whenever a pass brings more than two rows."""
        if mxfp4_lean and quant != "mxfp4":
            raise ValueError(f"mxfp4_lean=True drops the bf16 copies of the MXFP4 matrices: it needs weight_quant='mxfp4', not {quant!r}")
        self.mxfp4_lean = bool(mxfp4_lean)
        if mxfp6_lean and quant != "mxfp6":
            raise ValueError(f"mxfp6_lean=True drops the bf16 copies of the MXFP6 matrices: it needs weight_quant='mxfp6', not {quant!r}")
        self.mxfp6_lean = bool(mxfp6_lean)
        self._lean_dropped: List[Dict[str, object]] = []      # lean_report(): {"name", "n", "k", "bytes"} per matrix that has no bf16 copy
        if mxfp4_row_batch and quant != "mxfp4":
            raise ValueError(f"mxfp4_row_batch=True serves the MXFP4 companions on the row-batched path: it needs weight_quant='mxfp4', not {quant!r}")
        if mxfp4_row_batch and cfg.hidden > MXFP4_ROWS_MAX_HIDDEN:
            raise ValueError(f"mxfp4_row_batch=True serves LLM hidden sizes up to {MXFP4_ROWS_MAX_HIDDEN}, not {cfg.hidden}: beyond, the SwiGLU pair "
                             "would need a three-way K split, which the row-batched step's partials workspace has no room for")
        self.mxfp4_row_batch = bool(mxfp4_row_batch)
        if mxfp6_row_batch and quant != "mxfp6":
            raise ValueError(f"mxfp6_row_batch=True serves the MXFP6 companions on the row-batched path: it needs weight_quant='mxfp6', not {quant!r}")
        if mxfp6_row_batch and cfg.hidden > MXFP6_ROWS_MAX_HIDDEN:
            raise ValueError(f"mxfp6_row_batch=True serves LLM hidden sizes up to {MXFP6_ROWS_MAX_HIDDEN}, not {cfg.hidden}: beyond, the SwiGLU pair "
                             "would need a three-way K split, which the row-batched step's partials workspace has no room for")
        self.mxfp6_row_batch = bool(mxfp6_row_batch)
        self.cfg, self.device, self.wdtype = cfg, torch.device(device), wdtype
        if quant is not None and quant not in WEIGHT_FORMATS:
            raise ValueError(f"weight_quant {quant!r}: only None, " + " or ".join(f"{name!r} ({f.what})" for name, f in WEIGHT_FORMATS.items()) +
                             ", decode GEMVs, is built")
        if quant is not None and wdtype != torch.bfloat16:
            raise ValueError(f"weight_quant={quant!r} keeps bf16 copies for the GEMM-shaped uses: torch_dtype must be bfloat16")
        if prequant and quant != "nf4":
            raise ValueError(f"a pre-quantized bitsandbytes NF4 checkpoint runs as weight_quant='nf4', not {quant!r}")
        self.quant = quant
        self._pre = dict(prequant or {})
        self._fp8_names = set(fp8_matrix_names(cfg)) if quant is not None else set()     # the matrices that get a companion
        self.wdt = _wdt(wdtype)
        # the descriptors' wdt: VV_WQ_NF4 / VV_WQ_MXFP4 / VV_WQ_MXFP6 mark their vv_w8 companions as NF4 / MXFP4 / MXFP6 (vv_hip.h); self.wdt stays the plain matrix dtype
        self.desc_wdt = self.wdt | (WEIGHT_FORMATS[quant].wq if quant else 0)
        # vv_llm / vv_head: VV_WQ_FRAG4 / VV_WQ_FRAG6 say their layers' f_* copies hold the VV_MXFP4_FRAG / VV_MXFP6_FRAG form (never a bf16 fragment copy)
        self.desc_wdt_rows = self.desc_wdt | (L.VV_WQ_FRAG4 if self.mxfp4_row_batch else 0) | (L.VV_WQ_FRAG6 if self.mxfp6_row_batch else 0)
        self._keep: List[object] = []     # tensors / ctypes arrays that must outlive the descriptors
        # the fragment-major copies (ensure_frag) live here: one dict object shared by every fork, as the ctypes layer arrays they are
        # written into are, so they are built once per process whichever fork asks first
        # mxfp4_* / mxfp6_*: the VRAM record of the VV_MXFP4_FRAG / VV_MXFP6_FRAG copies - weights copied, bytes they take (0.5 + 1 / 32 = 0.53125,
        # 0.75 + 1 / 32 = 0.78125 B per weight)
        self._frag_state: Dict[str, object] = {"done": False, "tensors": [], "mxfp4_weights": 0, "mxfp4_bytes": 0, "mxfp6_weights": 0, "mxfp6_bytes": 0}
        self._sd = sd
        self.state_tensors: Dict[str, List[torch.Tensor]] = {"acoustic_dec": [], "semantic_enc": []}
        # every streaming-state tensor (conv left contexts, mixer histories) is a 256-byte aligned view into ONE arena, so the
        # engine can snapshot / roll back the whole speech state with a single copy (speculative frame launch)
        self._state_arena = torch.zeros(1 << 21, dtype=torch.float32, device=self.device)
        self._state_used = 0
        self._build_llm()
        self._build_head()
        self.dec = self._build_convnet("model.acoustic_tokenizer.decoder.", decoder=True, filters=cfg.ac_dec_filters,
                                       ratios=cfg.ac_ratios, depths_enc=cfg.ac_depths, dim=cfg.ac_dim, eps=cfg.ac_eps,
                                       state_key="acoustic_dec" if streaming_state else None)
        self.sem = self._build_convnet("model.semantic_tokenizer.encoder.", decoder=False, filters=cfg.sem_filters,
                                       ratios=cfg.sem_ratios, depths_enc=cfg.sem_depths, dim=cfg.sem_dim, eps=cfg.sem_eps,
                                       state_key="semantic_enc" if streaming_state else None)
        self.ac_enc = self._build_convnet("model.acoustic_tokenizer.encoder.", decoder=False, filters=cfg.ac_filters,
                                          ratios=cfg.ac_ratios, depths_enc=cfg.ac_depths, dim=cfg.ac_dim, eps=cfg.ac_eps,
                                          state_key=None)     # voice prompts are encoded whole (non-streaming)
        self.ac_conn = self._build_connector("model.acoustic_connector.", cfg.ac_dim)
        self.sem_conn = self._build_connector("model.semantic_connector.", cfg.sem_dim)
        self.speech_scale = float(sd["model.speech_scaling_factor"].float().item())
        self.speech_bias = float(sd["model.speech_bias_factor"].float().item())
        self._sd = None
        self._pre = {}

    # ---- helpers -------------------------------------------------------------------------------------------------
    @staticmethod
    def _aligned(t: torch.Tensor) -> torch.Tensor:
        # the streaming / matrix-core kernels need 16-byte aligned rows; a view into a packed blob may not be
        return t if t.data_ptr() % 256 == 0 else t.clone()

    def _mat(self, t: torch.Tensor) -> torch.Tensor:
        t = self._aligned(t.detach().to(device=self.device, dtype=self.wdtype).contiguous())
        self._keep.append(t)
        return t

    def _w(self, key: str) -> torch.Tensor:
        """A weight as the checkpoint holds it: the plain tensor, or for a pre-quantized bnb matrix its bf16 effective values (vv_nf4_import,
        no companion) in its quant_state shape."""
        r = self._pre.get(key)
        if r is None:
            return self._sd[key]
        from .bnb import import_nf4
        return import_nf4([r], self.device, companion=False)[0].view(r.shape)

    def _mat_q_keys(self, keys: List[str], quantise: bool, lean: Optional[str] = None):
        """_mat_q of the named matrices stacked along N (one key, or q / k / v for the fused [q|k|v] matrix).  Matrices that a pre-quantized
        checkpoint holds in bnb form are imported as they are - with the VV_NF4 companion when `quantise` and every part fits it exactly; a
        companion-set matrix that such a checkpoint holds unquantized runs bf16, without a companion (it is not quantised on the fly)."""
        if not self._pre:
            t = self._sd[keys[0]] if len(keys) == 1 else torch.cat([self._sd[k] for k in keys], dim=0)
            return self._mat_q(t, quantise, lean)
        w8 = L.W8()
        parts = [self._pre.get(k) for k in keys]
        if all(p is not None for p in parts):
            from .bnb import import_nf4
            comp = quantise and all(p.companion_exact() for p in parts)
            w, packed, scales = import_nf4(parts, self.device, companion=comp)
            if comp:
                self._keep.append(packed)
                w8.q, w8.scale = L.ptr(packed), L.ptr(self._vec(scales))
            return self._mat(w), w8
        t = torch.cat([self._w(k).to(self.device, self.wdtype) for k in keys], dim=0)
        return self._mat(t), w8

    def _mat_q(self, t: torch.Tensor, quantise: bool, lean: Optional[str] = None):
        """(bf16 matrix, vv_w8 companion) in the model's format (WEIGHT_FORMATS): the companion holds the codes and scales in the format's layout,
        the bf16 copy the effective weights - exact in bf16 in every format (fp8: power-of-two row scales; nf4: bf16(table[code] * absmax);
        mxfp4 / mxfp6: value(code) * 2^(e - 127)).  A matrix whose K the format's block does not divide gets no companion.  lean (a name for
        lean_report, mxfp4 / mxfp6 only): the bf16 copy is not made - (None, companion); the effective matrix lives while the codes are packed."""
        w8 = L.W8()
        f = WEIGHT_FORMATS[self.quant] if quantise and self.quant else None
        if f is None or (f.block and t.shape[1] % f.block):
            return self._mat(t), w8
        # the blockwise formats quantise the bf16 weight, widened; fp8 the matrix as given
        codes, scales, eff = f.quantize(t.to(self.device) if f.block is None else t.to(device=self.device, dtype=torch.bfloat16))
        if f.pack:
            codes, scales = f.pack(codes, scales)
        codes, scales = self._aligned(codes.to(self.device)), self._aligned(scales.to(self.device))
        self._keep += [codes, scales]
        w8.q, w8.scale = L.ptr(codes), L.ptr(scales)      # scale: fp32 scales (fp8, nf4) or the address of the E8M0 scale BYTES (vv_hip.h)
        if lean is not None and self.quant in ("mxfp4", "mxfp6"):
            n, k = t.shape
            self._lean_dropped.append({"name": lean, "n": int(n), "k": int(k), "bytes": 2 * int(n) * int(k)})
            return None, w8
        return self._mat(eff), w8

    def _vec(self, t: torch.Tensor) -> torch.Tensor:
        t = self._aligned(t.detach().to(device=self.device, dtype=torch.float32).contiguous())
        self._keep.append(t)
        return t

    def _state_zeros(self, rows: int, ch: int) -> torch.Tensor:
        n = rows * ch
        if self._state_used + n > self._state_arena.numel():
            raise ValueError("streaming-state arena too small for this tokenizer configuration")
        t = self._state_arena[self._state_used: self._state_used + n].view(rows, ch)
        self._state_used += (n + 63) // 64 * 64
        return t

    def fork(self) -> "DeviceWeights":
        """A second set of descriptors over the SAME device weights with a streaming-state arena of its own (a lane of a lock-step batch,
        a concurrent dialogue): nothing is re-laid-out or copied except the few KB of ctypes descriptors that carry state pointers."""
        w = object.__new__(DeviceWeights)
        w.__dict__.update(self.__dict__)
        w._keep = list(self._keep)
        w._state_arena = torch.zeros_like(self._state_arena)
        old0, new0 = self._state_arena.data_ptr(), w._state_arena.data_ptr()

        def reloc(p):
            return None if not p else new0 + (int(p) - old0)

        def fork_net(net: "L.ConvNet") -> "L.ConvNet":
            n2 = L.ConvNet.from_buffer_copy(net)
            for i in range(net.n_stages):
                n2.sample[i].state = reloc(net.sample[i].state)
                nb = net.n_blocks[i]
                if nb > 0:
                    arr = (L.Block * nb)()
                    C.memmove(arr, net.blocks[i], C.sizeof(L.Block) * nb)
                    for j in range(nb):
                        arr[j].hist = reloc(arr[j].hist)
                        arr[j].hs = reloc(arr[j].hs)
                    w._keep.append(arr)
                    n2.blocks[i] = C.cast(arr, C.POINTER(L.Block))
            n2.head.state = reloc(net.head.state)
            return n2

        w.dec, w.sem = fork_net(self.dec), fork_net(self.sem)
        f32 = 4
        w.state_tensors = {k: [w._state_arena[(t.data_ptr() - old0) // f32: (t.data_ptr() - old0) // f32 + t.numel()].view_as(t) for t in v]
                           for k, v in self.state_tensors.items()}
        return w

    @staticmethod
    def frag_major(w: torch.Tensor) -> Optional[torch.Tensor]:
        """[N, K] bf16 -> the fragment-major copy [N / 16][K / 32][4][16][8] (include/vv_hip.h, vv_llm_layer.f_*): element (16 g + n, 32 j + 8 c + e)
        at ((g * K/32 + j) * 64 + 16 c + n) * 8 + e, one matrix-core B fragment per KB of contiguous memory."""
        n, k = w.shape
        if n % 16 or k % 32 or w.dtype != torch.bfloat16:
            return None
        return w.view(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).contiguous()

    @staticmethod
    def frag_major_fp8(q: torch.Tensor) -> Optional[torch.Tensor]:
        """[N, K] e4m3fn codes (uint8) -> the fp8 fragment-major copy [N / 16][K / 64][64 lanes][16 B] (include/vv_hip.h, vv_llm_layer.f_*): lane
        16 c + n of 64-wide k step j of row group g holds W[16 g + n][64 j + 8 c ..+8] then W[16 g + n][64 j + 32 + 8 c ..+8], i.e. element
        (16 g + n, 64 j + 32 h + 8 c + e) at ((g * K/64 + j) * 64 + 16 c + n) * 16 + 8 h + e."""
        n, k = q.shape
        if n % 16 or k % 64 or q.dtype != torch.uint8:
            return None
        return q.view(n // 16, 16, k // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).contiguous()

    @staticmethod
    def frag_major_mxfp4(codes: torch.Tensor, scales: torch.Tensor) -> Optional[torch.Tensor]:
        """(e2m1 codes uint8 [N, K], E8M0 scale bytes uint8 [N, K / 32]) -> the VV_MXFP4_FRAG form (include/vv_hip.h) as ONE uint8 tensor: the
        codes [N / 16][K / 128][64 lanes][16 B] - nibble i of dword h of lane 16 c + n of 128-wide step J of row group g is code
        (16 g + n, 128 J + 32 h + 8 c + i) - then, at byte offset N K / 2, the scale bytes [N / 16][K / 128][16 rows][4 B] - byte h of the dword
        of (g, J, n) is the byte of block 4 J + h of row 16 g + n.  None when N % 16 or K % 128."""
        n, k = codes.shape
        if n % 16 or k % 128 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or tuple(scales.shape) != (n, k // MXFP4_BLOCK):
            return None
        c = codes.view(n // 16, 16, k // 128, 4, 4, 4, 2).permute(0, 2, 4, 1, 3, 5, 6)       # [g, n, J, h, c, byte, nibble] -> [g, J, c, n, h, byte, nibble]
        packed = (c[..., 0] | (c[..., 1] << 4)).contiguous().view(-1)
        sb = scales.view(n // 16, 16, k // 128, 4).permute(0, 2, 1, 3).contiguous().view(-1)  # [g, J, n, h]
        return torch.cat([packed, sb])

    @staticmethod
    def unfrag_mxfp4(f: torch.Tensor, n: int, k: int):
        """Inverse of frag_major_mxfp4: (codes uint8 [N, K], scale bytes uint8 [N, K / 32])."""
        b = f[: n * k // 2].view(n // 16, k // 128, 4, 16, 4, 4)                              # [g, J, c, n, h, byte]
        c = torch.stack([b & 15, b >> 4], dim=-1)                                             # ... nibble
        codes = c.permute(0, 3, 1, 4, 2, 5, 6).reshape(n, k).contiguous()
        scales = f[n * k // 2:].view(n // 16, k // 128, 16, 4).permute(0, 2, 1, 3).reshape(n, k // MXFP4_BLOCK).contiguous()
        return codes, scales

    @staticmethod
    def frag_major_mxfp6(codes: torch.Tensor, scales: torch.Tensor) -> Optional[torch.Tensor]:
        """(e2m3 codes uint8 [N, K] in 0..63, E8M0 scale bytes uint8 [N, K / 32]) -> the VV_MXFP6_FRAG form (include/vv_hip.h) as ONE uint8 tensor.
        Lane 16 c + n of 128-wide step J of row group g owns block 4 J + c of row 16 g + n: its 24 bytes (code i in bits 6 i .. 6 i + 5, the
        string of VV_MXFP6) are split into plane A [N / 16][K / 128][64 lanes][16 B] (bytes 0..15) and, at byte offset N K / 2, plane B
        [N / 16][K / 128][64 lanes][8 B] (bytes 16..23); then, at N K 3 / 4, the scale bytes [N / 16][K / 128][16 rows][4 B] - byte c of the
        dword of (g, J, n) is the byte of block 4 J + c of row 16 g + n.  None when N % 16 or K % 128."""
        n, k = codes.shape
        if n % 16 or k % 128 or codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or tuple(scales.shape) != (n, k // MXFP6_BLOCK):
            return None
        dev = codes.device
        bits = (codes.view(n // 16, 16, k // 128, 4, 32, 1) >> torch.arange(6, device=dev, dtype=torch.uint8)) & 1      # [g, n, J, c, element, bit]
        by = (bits.reshape(n // 16, 16, k // 128, 4, 24, 8) << torch.arange(8, device=dev, dtype=torch.uint8)).sum(dim=-1, dtype=torch.uint8)
        by = by.permute(0, 2, 3, 1, 4)                                                          # [g, J, c, n, 24 bytes]: lane 16 c + n
        sb = scales.view(n // 16, 16, k // 128, 4).permute(0, 2, 1, 3)                          # [g, J, n, c]
        return torch.cat([by[..., :16].reshape(-1), by[..., 16:].reshape(-1), sb.reshape(-1)])

    @staticmethod
    def unfrag_mxfp6(f: torch.Tensor, n: int, k: int):
        """Inverse of frag_major_mxfp6: (codes uint8 [N, K], scale bytes uint8 [N, K / 32])."""
        g, kj = n // 16, k // 128
        by = torch.cat([f[: n * k // 2].view(g, kj, 4, 16, 16), f[n * k // 2: n * k * 3 // 4].view(g, kj, 4, 16, 8)], dim=-1)      # [g, J, c, n, 24 bytes]
        bits = ((by[..., None] >> torch.arange(8, device=f.device, dtype=torch.uint8)) & 1).reshape(g, kj, 4, 16, 32, 6)
        codes = (bits << torch.arange(6, device=f.device, dtype=torch.uint8)).sum(dim=-1, dtype=torch.uint8)                    # [g, J, c, n, element]
        codes = codes.permute(0, 3, 1, 2, 4).reshape(n, k).contiguous()
        scales = f[n * k * 3 // 4:].view(g, kj, 16, 4).permute(0, 2, 1, 3).reshape(n, k // MXFP6_BLOCK).contiguous()
        return codes, scales

    def ensure_frag(self) -> None:
        """Fragment-major copies of the LLM's and the diffusion head's per-frame matrices for the row-batched decode step (rowbatch.py): built
        once per process (for this weight set and all its forks), on first use, next to the row-major matrices (which the prefill GEMMs and the
        1..4-row GEMVs keep using).  bf16: copies of the bf16 matrices, +2.9 GB at 1.5B.  weight_quant="fp8": copies of the e4m3 codes of the
        matrices' fp8 companions instead (+1.45 GB at 1.5B) - a layer's f_* then points at fp8 codes (the vv_llm_layer rule); a matrix whose
        shape the fp8 form cannot take (N % 16, K % 64) gets no copy and keeps the row-major fallback.  weight_quant="mxfp4" with
        mxfp4_row_batch: the VV_MXFP4_FRAG form of the MXFP4 companions (frag_major_mxfp4: +0.53 B per copied weight, recorded in
        _frag_state["mxfp4_weights"] / ["mxfp4_bytes"] and counted by nbytes()), never a bf16 copy: a matrix without a companion or with
        N % 16 / K % 128 keeps f_* = NULL and the row-major bf16 fallback, and so does the head's gate / up pair beyond K = 2048 (MXFP4_ROWS_MOD_K:
        it is called with the adaLN prologue, which the MX rows kernel serves on whole rows only - a copy would never be read).
        weight_quant="mxfp6" with mxfp6_row_batch: the same with the VV_MXFP6_FRAG form (frag_major_mxfp6: +0.78 B per copied weight, recorded
        in _frag_state["mxfp6_weights"] / ["mxfp6_bytes"]), under the same two rules."""
        st = self._frag_state
        if st["done"] or self.wdtype != torch.bfloat16:
            return
        by_ptr = {t.data_ptr(): t for t in self._keep if isinstance(t, torch.Tensor)}
        mx = "mxfp4" if self.mxfp4_row_batch else "mxfp6" if self.mxfp6_row_batch else None      # the MX row-batch opt-in, if any: no bf16 copy then
        mx_frag, mx_unpack = (self.frag_major_mxfp4, unpack_mxfp4) if mx == "mxfp4" else (self.frag_major_mxfp6, unpack_mxfp6)

        def frag_of(p, w8, n, k):
            if mx:                              # MX companion: its codes and scale bytes, re-laid (the companion's own layout is pack_mxfp4's / pack_mxfp6's)
                packed, sb = by_ptr.get(int(w8.q or 0)), by_ptr.get(int(w8.scale or 0))
                if packed is None or sb is None or k % MXFP4_BLOCK:
                    return None
                f = mx_frag(*mx_unpack(packed, sb, n, k))
                if f is None:
                    return None
                f = self._aligned(f)
                st["tensors"].append(f)
                st[mx + "_weights"] += n * k
                st[mx + "_bytes"] += f.numel()
                return f.data_ptr()
            if w8.q and self.quant == "fp8":    # fp8 companion: the copy is of its codes, or none (NF4: the bf16 effective matrix)
                t, fm = by_ptr.get(int(w8.q)), self.frag_major_fp8
            else:
                t, fm = (by_ptr.get(int(p)) if p else None), self.frag_major
            if t is None or tuple(t.shape) != (n, k):
                return None
            f = fm(t)
            if f is None:
                return None
            f = self._aligned(f)
            st["tensors"].append(f)
            return f.data_ptr()

        cfg = self.cfg
        qkvd = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        for l in range(cfg.layers):
            lay = self.llm.layer[l]
            lay.f_qkv = frag_of(lay.wqkv, lay.q_qkv, qkvd, cfg.hidden)
            lay.f_o = frag_of(lay.wo, lay.q_o, cfg.hidden, cfg.heads * cfg.head_dim)
            lay.f_gate = frag_of(lay.wgate, lay.q_gate, cfg.inter, cfg.hidden)
            lay.f_up = frag_of(lay.wup, lay.q_up, cfg.inter, cfg.hidden)
            lay.f_down = frag_of(lay.wdown, lay.q_down, cfg.hidden, cfg.inter)
        for l in range(cfg.head_layers):
            lay = self.head.layer[l]
            if mx and cfg.head_hidden > MXFP4_ROWS_MOD_K:     # no MX rows route takes the modulated pair at this K: no copy
                lay.f_gate = lay.f_up = None
            else:
                lay.f_gate = frag_of(lay.wgate, lay.q_gate, cfg.head_ffn, cfg.head_hidden)
                lay.f_up = frag_of(lay.wup, lay.q_up, cfg.head_ffn, cfg.head_hidden)
            lay.f_down = frag_of(lay.wdown, lay.q_down, cfg.head_hidden, cfg.head_ffn)
        st["done"] = True

    def state_blob(self) -> torch.Tensor:
        """All streaming state of the speech path as one flat fp32 tensor."""
        return self._state_arena[: max(self._state_used, 64)]

    def _zeros(self, *shape) -> torch.Tensor:
        t = torch.zeros(*shape, dtype=torch.float32, device=self.device)
        self._keep.append(t)
        return t

    def lean_report(self) -> List[Dict[str, object]]:
        """The matrices an mxfp4_lean / mxfp6_lean model holds as MX codes alone: [{"name", "n", "k", "bytes"}], bytes = 2 n k = the bf16 copy that
        was not uploaded (nbytes() of the same model without the keyword is larger by exactly their sum).  Empty without the mode."""
        return [dict(d) for d in self._lean_dropped]

    def nbytes(self) -> int:
        ts = [t for t in self._keep if isinstance(t, torch.Tensor)] + list(self._frag_state["tensors"])
        return sum(t.numel() * t.element_size() for t in ts)

    # ---- Qwen2 ---------------------------------------------------------------------------------------------------
    def _build_llm(self):
        cfg, sd = self.cfg, self._sd
        p = "model.language_model."
        self.embed = self._mat(self._w(p + "embed_tokens.weight"))
        has_head = "lm_head.weight" in sd or "lm_head.weight" in self._pre
        self.lm_head = self.embed if (cfg.tie or not has_head) else self._mat(self._w("lm_head.weight"))
        layers = (L.LlmLayer * cfg.layers)()
        # lean: all of the LLM's matrices or none (csrc/vv_model.hip takes a model whose five pointers are NULL in every layer) - every one of
        # them must be a shape the GEMM on the codes takes: N % 16 == 0, K % 128 == 0
        qd, qkvd = cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
        lean = (self.mxfp4_lean or self.mxfp6_lean) and not (cfg.hidden % 128 or cfg.inter % 128 or qd % 128 or qkvd % 16)
        for l in range(cfg.layers):
            q = f"{p}layers.{l}."
            qz = self.quant is not None
            lay = layers[l]
            wqkv, lay.q_qkv = self._mat_q_keys([q + f"self_attn.{n}_proj.weight" for n in "qkv"], qz, q + "self_attn.qkv_proj.weight" if lean else None)
            bqkv = self._vec(torch.cat([sd[q + "self_attn.q_proj.bias"], sd[q + "self_attn.k_proj.bias"],
                                        sd[q + "self_attn.v_proj.bias"]], dim=0))
            lay.ln1 = L.ptr(self._vec(sd[q + "input_layernorm.weight"]))
            lay.ln2 = L.ptr(self._vec(sd[q + "post_attention_layernorm.weight"]))
            lay.wqkv, lay.bqkv = L.ptr(wqkv), L.ptr(bqkv)
            for field, qf, key in (("wo", "q_o", "self_attn.o_proj.weight"), ("wgate", "q_gate", "mlp.gate_proj.weight"),
                                   ("wup", "q_up", "mlp.up_proj.weight"), ("wdown", "q_down", "mlp.down_proj.weight")):
                wm, w8 = self._mat_q_keys([q + key], qz, q + key if lean else None)
                setattr(lay, field, L.ptr(wm))
                setattr(lay, qf, w8)
        # Qwen2RotaryEmbedding.compute_default_rope_parameters, same fp32 ops as the reference stack
        inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.float) / cfg.head_dim))
        self.inv_freq = self._vec(inv_freq)
        m = L.Llm()
        m.wdt, m.hidden, m.inter, m.layers = self.desc_wdt_rows, cfg.hidden, cfg.inter, cfg.layers
        m.heads, m.kv_heads, m.head_dim, m.rms_eps = cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.rms_eps
        m.inv_freq = L.ptr(self.inv_freq)
        m.final_norm = L.ptr(self._vec(sd[p + "norm.weight"]))
        m.layer = C.cast(layers, C.POINTER(L.LlmLayer))
        self._keep.append(layers)
        self.llm = m

    # ---- diffusion head ------------------------------------------------------------------------------------------
    def _build_head(self):
        cfg, sd = self.cfg, self._sd
        p = "model.prediction_head."
        layers = (L.HeadLayer * cfg.head_layers)()
        for l in range(cfg.head_layers):
            q = f"{p}layers.{l}."
            lay = layers[l]
            lay.norm_w = L.ptr(self._vec(sd[q + "norm.weight"]))
            for field, qf, key in (("wgate", "q_gate", "ffn.gate_proj.weight"), ("wup", "q_up", "ffn.up_proj.weight"),
                                   ("wdown", "q_down", "ffn.down_proj.weight")):
                wm, w8 = self._mat_q_keys([q + key], self.quant is not None)
                setattr(lay, field, L.ptr(wm))
                setattr(lay, qf, w8)
            lay.adaln = L.ptr(self._mat(self._w(q + "adaLN_modulation.1.weight")))
        h = L.Head()
        h.wdt, h.D, h.ffn, h.layers, h.latent, h.cond_dim = self.desc_wdt_rows, cfg.head_hidden, cfg.head_ffn, cfg.head_layers, cfg.latent, cfg.hidden
        h.eps = cfg.head_eps
        h.noisy_proj = L.ptr(self._mat(self._w(p + "noisy_images_proj.weight")))
        h.cond_proj = L.ptr(self._mat(self._w(p + "cond_proj.weight")))
        h.final_adaln = L.ptr(self._mat(self._w(p + "final_layer.adaLN_modulation.1.weight")))
        h.final_linear = L.ptr(self._mat(self._w(p + "final_layer.linear.weight")))
        h.layer = C.cast(layers, C.POINTER(L.HeadLayer))
        self._keep.append(layers)
        # G = [P F ; F] (fp32, built once in fp64 from the matrices the kernels stream: bf16-rounded in bf16 mode): every solver-step
        # boundary - final linear, CFG, DPM-Solver++ update, next noisy_images_proj, all linear in the modulated hidden state - is
        # one GEMV over it (csrc/vv_fused.hip); P (F y) == (P F) y up to fp32 rounding
        P = self._w(p + "noisy_images_proj.weight").to(device=self.device, dtype=self.wdtype).double()
        F = self._w(p + "final_layer.linear.weight").to(device=self.device, dtype=self.wdtype).double()
        self.head_g = self._vec(torch.cat([P @ F, F], dim=0).float())
        h.fused_g = L.ptr(self.head_g)
        self.head = h
        self.t_mlp0 = self._mat(self._w(p + "t_embedder.mlp.0.weight"))
        self.t_mlp2 = self._mat(self._w(p + "t_embedder.mlp.2.weight"))

    # ---- conv tokenizers -----------------------------------------------------------------------------------------
    def _conv(self, w: torch.Tensor, b: torch.Tensor, stride: int, transposed: bool, state_key) -> L.Conv:
        c = L.Conv()
        if transposed:
            cin, cout, k = w.shape
            s = stride
            assert k == 2 * s, "SConvTranspose1d with k != 2*stride is not on the shipped path"
            w4 = w.reshape(cin, cout, 2, s).flip(2)                     # [ci, co, j, r]: j=0 -> taps r+s (previous input)
            wl = w4.permute(3, 1, 2, 0).reshape(s * cout, 2 * cin)      # [(r, co), (j, ci)]
            bl = b.repeat(s)
            ctx = 1
        else:
            cout, cin, k = w.shape
            wl = w.permute(0, 2, 1).reshape(cout, k * cin)              # [co, (tap, ci)]
            bl = b
            ctx = k - stride
        c.w, c.b = L.ptr(self._mat(wl)), L.ptr(self._vec(bl))
        c.cin, c.cout, c.kk, c.stride, c.transposed = cin, cout, k, stride, int(transposed)
        if state_key is not None and ctx > 0:
            st = self._state_zeros(ctx, cin)
            self.state_tensors[state_key].append(st)
            c.state = L.ptr(st)
        else:
            c.state = None
        return c

    def _blocks(self, prefix: str, n: int, ch: int, state_key):
        sd = self._sd
        arr = (L.Block * max(n, 1))()
        for j in range(n):
            q = f"{prefix}{j}."
            b = arr[j]
            b.gamma = L.ptr(self._vec(sd[q + "gamma"]))
            b.ffn_gamma = L.ptr(self._vec(sd[q + "ffn_gamma"]))
            b.norm_w = L.ptr(self._vec(sd[q + "norm.weight"]))
            b.ffn_norm_w = L.ptr(self._vec(sd[q + "ffn_norm.weight"]))
            b.dw_w = L.ptr(self._vec(sd[q + "mixer.conv.conv.conv.weight"].reshape(ch, 7)))
            b.dw_b = L.ptr(self._vec(sd[q + "mixer.conv.conv.conv.bias"]))
            qz = state_key is not None and (q + "ffn.linear1.weight") in self._fp8_names
            w1m, b.q_w1 = self._mat_q_keys([q + "ffn.linear1.weight"], qz)
            w2m, b.q_w2 = self._mat_q_keys([q + "ffn.linear2.weight"], qz)
            b.w1, b.b1 = L.ptr(w1m), L.ptr(self._vec(sd[q + "ffn.linear1.bias"]))
            b.w2, b.b2 = L.ptr(w2m), L.ptr(self._vec(sd[q + "ffn.linear2.bias"]))
            if state_key is not None:
                h = self._state_zeros(6, ch)
                self.state_tensors[state_key].append(h)
                b.hist = L.ptr(h)
                if ch == 2048 and not b.q_w1.q:
                    # the one-row stage: the history part of the depthwise conv is carried as state (hs = sum_k<6 tap_k * hist_k, zero with
                    # hist, inside the same arena so reset / snapshot / rollback cover it) and the newest row's tap is packed
                    b.dw_last = L.ptr(self._vec(sd[q + "mixer.conv.conv.conv.weight"].reshape(ch, 7)[:, 6].contiguous()))
                    b.hs = L.ptr(self._state_zeros(1, ch))
            else:
                b.hist = None
        self._keep.append(arr)
        return arr

    def _build_convnet(self, prefix, decoder, filters, ratios, depths_enc, dim, eps, state_key) -> L.ConvNet:
        sd = self._sd
        n = len(depths_enc)
        if n > L.VV_MAX_STAGES:
            raise ValueError("too many tokenizer stages")
        net = L.ConvNet()
        net.wdt, net.n_stages, net.eps = self.desc_wdt, n, eps
        if decoder:
            depths = list(reversed(depths_enc))
            for i in range(n):
                ch = filters * 2 ** (n - 1 - i)
                if i == 0:
                    q = prefix + "upsample_layers.0.0.conv.conv."
                    net.sample[i] = self._conv(self._w(q + "weight"), sd[q + "bias"], 1, False, state_key)
                else:
                    q = prefix + f"upsample_layers.{i}.0.convtr.convtr."
                    net.sample[i] = self._conv(self._w(q + "weight"), sd[q + "bias"], ratios[i - 1], True, state_key)
                net.n_blocks[i] = depths[i]
                arr = self._blocks(prefix + f"stages.{i}.", depths[i], ch, state_key)
                net.blocks[i] = C.cast(arr, C.POINTER(L.Block))
        else:
            rr = list(reversed(ratios))
            for i in range(n):
                ch = filters * 2 ** i
                q = prefix + f"downsample_layers.{i}.0.conv.conv."
                net.sample[i] = self._conv(self._w(q + "weight"), sd[q + "bias"], 1 if i == 0 else rr[i - 1], False, state_key)
                net.n_blocks[i] = depths_enc[i]
                arr = self._blocks(prefix + f"stages.{i}.", depths_enc[i], ch, state_key)
                net.blocks[i] = C.cast(arr, C.POINTER(L.Block))
        q = prefix + "head.conv.conv."
        net.head = self._conv(self._w(q + "weight"), sd[q + "bias"], 1, False, state_key)
        return net

    def _build_connector(self, prefix, din) -> L.Connector:
        sd = self._sd
        c = L.Connector()
        c.wdt, c.din, c.hidden = self.wdt, din, self.cfg.hidden
        c.fc1, c.b1 = L.ptr(self._mat(self._w(prefix + "fc1.weight"))), L.ptr(self._vec(sd[prefix + "fc1.bias"]))
        c.norm_w = L.ptr(self._vec(sd[prefix + "norm.weight"]))
        c.fc2, c.b2 = L.ptr(self._mat(self._w(prefix + "fc2.weight"))), L.ptr(self._vec(sd[prefix + "fc2.bias"]))
        return c

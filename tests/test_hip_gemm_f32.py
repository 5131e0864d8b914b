"""The fp32 LDS-tiled GEMM (csrc/vv_kernels.hip, gemm_kernel<WT, dual, vec, TMT, TNT>) and the resampling convs' skinny GEMM (csrc/vv_convffn.hip,
skinny_kernel<NST, NB>) against plain fp64, per output tile - through the C ABI only, no engine, no weights.

Each case first asks `vv_linear_route` which kernel its arguments take and asserts the instantiation it means to test: the 16 instantiations
of gemm_kernel (`gemm_f32<w=f32|bf16,dual=0|1,vec=0|1,tile=32|64>`) and the 7 of skinny_kernel (`skinny<nst=N,nb=N>`) are each reached by at least
one case (table below).  Case, layout, NaN gaps and guard rows, the two bit-identical runs and the untouched inputs are those of
tests/test_hip_mfma_gemm.py; what that file lacks is added here: fp32 weights, activations that are NOT rounded to bf16, operands a few bytes
past a 16-byte boundary and row pitches that are no multiple of 4.

Reference: plain torch fp64 on the operands as the device receives them (`ref_linear_fp64`); rows may overlap (ldx < k), as a dense conv reads
its padded input in place (`test_overlapping_rows_are_the_convs`, CPU, holds that reading against conv1d / conv_transpose1d).
  gemm_f32  no rounding anywhere: prologue, product and epilogue in fp64.
  skinny    x rounded to bf16 once (pack2 = round to nearest even), bf16 weights, the bias added in fp64.
Three figures per case: global rel RMS, the worst aligned tile a workgroup owns (32 x 32 for gemm_f32 - the 64 x 64 kernel is judged on the finer
grid too - and 16 x 16 for skinny) and the worst row.  The row figure counts only where a row has at least 8 columns: with n = 1 a row is one
value and its relative error is unbounded (the fp32 stand-in alone gives 5.7e-4 for one row of the 3200 x 1 x 224 case against 1.5e-7 for its
worst tile); narrower cases are held to the global and tile figures.

Bars: one constant per class (BAR), held on the CPU by `test_bars_sit_between_floor_and_dropped_step` for every case; derivation at BAR.

Measured on the MI355X, largest value over the class's cases, global / worst tile / worst row rel RMS against fp64
(profiles/gemm_f32_skinny_parity.txt):
  class     cases   bar      global / tile / row              bar / largest
  plain        77   1e-4     2.6e-6 / 3.3e-6 / 4.5e-6              22
  rms           8   1e-4     5.6e-7 / 6.3e-7 / 7.1e-7             141
  rms_mod       6   1e-4     5.7e-7 / 6.1e-7 / 7.1e-7             141
  silu          4   1e-4     1.4e-7 / 2.2e-7 / 1.9e-7             462
  skinny       23   1e-4     2.3e-7 / 2.7e-7 / 3.7e-7             271
No value is within a factor of ten of its bar.  The nearest, 4.5e-6 for one row of the K = 8960 SwiGLU call (g_f32_k8960_dual), 22 times below
1e-4, is the length of the chain: 8960 fp32 multiply-adds in a row, in both factors of the product, and the device gives the very figures of the
CPU chain stand-in there (2.59e-6 / 3.31e-6 / 4.46e-6).  Every other case of the file stays below 8e-7.  No kernel defect was found.

Instantiation -> case ids (generated: `python tests/test_hip_gemm_f32.py --table`; `test_docstring_table_is_current` keeps it so):
  gemm_f32<w=f32,dual=0,vec=0,tile=32>       g_f32_m9_n1_k7, g_f32_m9_n31_k17, g_f32_m17_n31_k7, g_f32_m17_n70_k17, ... (12 cases)
  gemm_f32<w=f32,dual=0,vec=1,tile=32>       g_f32_191tiles, g_f32_m9_n70_k20, g_f32_m17_n1_k224, g_f32_m33_n1_k56, ... (25 cases)
  gemm_f32<w=f32,dual=1,vec=0,tile=32>       g_f32_dual_novec_w2, g_f32_dual_novec_k
  gemm_f32<w=f32,dual=1,vec=1,tile=32>       g_f32_k8960_dual, g_f32_dual_vec, g_f32_rms_swiglu, g_f32_swiglu_gate_res
  gemm_f32<w=f32,dual=0,vec=0,tile=64>       g_f32_t64_novec
  gemm_f32<w=f32,dual=0,vec=1,tile=64>       g_f32_t64_vec, g_f32_192tiles
  gemm_f32<w=f32,dual=1,vec=0,tile=64>       g_f32_t64_dual_novec, g_f32_t64_rms_dual
  gemm_f32<w=f32,dual=1,vec=1,tile=64>       g_f32_t64_dual_vec
  gemm_f32<w=bf16,dual=0,vec=0,tile=32>      g_bf16_m9_n9_k7, g_bf16_m9_n33_k17, g_bf16_m17_n33_k7, g_bf16_m17_n130_k17, ... (12 cases)
  gemm_f32<w=bf16,dual=0,vec=1,tile=32>      g_bf16_191tiles, g_bf16_m9_n130_k20, g_bf16_m17_n9_k1000, g_bf16_m33_n9_k56, ... (22 cases)
  gemm_f32<w=bf16,dual=1,vec=0,tile=32>      g_bf16_dual_novec_w2, g_bf16_dual_novec_k
  gemm_f32<w=bf16,dual=1,vec=1,tile=32>      g_bf16_k1000_dual, g_bf16_dual_vec, g_bf16_rms_swiglu, g_bf16_swiglu_gate_res
  gemm_f32<w=bf16,dual=0,vec=0,tile=64>      g_bf16_t64_novec
  gemm_f32<w=bf16,dual=0,vec=1,tile=64>      g_bf16_t64_vec, g_bf16_t64_rmsnow_mod, g_bf16_192tiles
  gemm_f32<w=bf16,dual=1,vec=0,tile=64>      g_bf16_t64_dual_novec
  gemm_f32<w=bf16,dual=1,vec=1,tile=64>      g_bf16_t64_dual_vec
  skinny<nst=1,nb=1>                         s_k128_m1603_overlap, s_k128_m1603_gap, s_k128_m2048_gap, s_frame_1600x64x128
  skinny<nst=2,nb=1>                         s_k256_m5_overlap, s_k256_m17_gap, s_frame_800x128x256
  skinny<nst=4,nb=1>                         s_k512_m37_overlap, s_k512_m200_gap, s_dec_200x512x512
  skinny<nst=8,nb=1>                         s_k1024_m16_overlap, s_k1024_m17_gap, s_dec_40x1280x1024, s_enc_200x256x1024
  skinny<nst=16,nb=1>                        s_k2048_m37_overlap, s_k2048_m5_gap, s_dec_8x2560x2048
  skinny<nst=20,nb=1>                        s_k2560_m17_overlap, s_k2560_m16_gap, s_enc_40x512x2560
  skinny<nst=20,nb=2>                        s_k5120_m37_overlap, s_k5120_m5_gap, s_enc_8x1024x5120
"""
import ctypes as C
import functools
import math
import os
import sys
import zlib

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_rms
from test_hip_mfma_gemm import DROP_MARGIN, FLOOR_HEADROOM, Case, _FAKE, _epilogue, _lib, _need_gpu, _prologue, _rel, _same_bits, bf16_round64, \
    built_kernels, fill_args, instantiations_of, layout, ref_linear_fp64, route_of, tile_row_errors

NAN = float("nan")
ROW_MIN_COLS = 8           # the row figure is taken only where a row has at least this many columns

# One constant per class, held for the global, the worst-tile and (n >= 8) the worst-row figure alike.  Chosen from the arithmetic, then checked
# against both conditions on the CPU (test_bars_sit_between_floor_and_dropped_step); never from what the device gives.
#   plain    gemm_f32 without a prologue.  Nothing is rounded to bf16 on either side, so the error is fp32 accumulation alone: one ascending
#            chain of K fused multiply-adds per output, <= ~ sqrt(K) 2^-24 of the sum's own rms for random signs - 5.6e-6 at K = 8960, the
#            longest the project uses (the chain stand-in gives 1.7e-6 global and 2.4e-6 for its worst row there, 2.6e-6 and 4.5e-6 through SwiGLU,
#            where both factors carry a chain) - and at most 7e-7 at every other K of the file.  An edge tile of one column or one row divides by a few reference values that can sit ~ 10x below rms.  1e-4,
#            the value of BAR["none"] and BAR["xb"] of tests/test_hip_mfma_gemm.py, is 8 x above the largest of these with room to spare,
#            and the cheapest dropped 16-wide step of the class (K = 8960: sqrt(16 / 8960) = 4.2e-2, measured 4.3e-2) is ~ 400x above it.
#   rms      RMSNorm (with or without a weight) in fp32 in front of the same chain: a mean of K squares, rsqrtf, one or two multiplies - a few
#            2^-24 per activation, no bf16 rounding that could flip, so the class behaves like plain: 1e-4.  K <= 1000 in this class: a dropped
#            step costs its tile >= sqrt(16 / 1000) = 1.3e-1.
#   rms_mod  two more fp32 operations (x (1 + scale) + shift) per activation: 1e-4 for the same reason.
#   silu     expf and a division per activation, ~ 2 ulp of fp32 each: 1e-4.
#   skinny   x is rounded to bf16 by the same round-to-nearest-even on both sides and the weights are bf16, so the products are exact in fp32
#            and the error is fp32 accumulation again: K / 4 per wave on the matrix core, four partial sums added in a fixed order; K <= 5120,
#            so <= sqrt(5120) 2^-24 = 4.3e-6.  1e-4; the cheapest dropped 32-wide step (K = 5120: sqrt(32 / 5120) = 7.9e-2, measured 7.3e-2)
#            is ~ 700x above it.
BAR = {"plain": 1e-4, "rms": 1e-4, "rms_mod": 1e-4, "silu": 1e-4, "skinny": 1e-4}


def _gemm(w, dual, vec, tile):
    return f"gemm_f32<w={w},dual={dual},vec={vec},tile={tile}>"


def _skinny(nst, nb):
    return f"skinny<nst={nst},nb={nb}>"


SKINNY_OF_K = {128: (1, 1), 256: (2, 1), 512: (4, 1), 1024: (8, 1), 2048: (16, 1), 2560: (20, 1), 5120: (20, 2)}
ALL_INSTANTIATIONS = [_gemm(w, d, v, t) for w in ("f32", "bf16") for t in (32, 64) for d in (0, 1) for v in (0, 1)] + \
                     [_skinny(*SKINNY_OF_K[k]) for k in sorted(SKINNY_OF_K)]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class FCase(Case):
    """A Case of tests/test_hip_mfma_gemm.py with fp32 activations and, new here, w: "f32" | "bf16" weights; off: {operand: elements} - x, w or
    w2 that many elements past its allocation's 16-byte boundary; ldx: any row pitch (ldx < k: overlapping rows; ldx >= k: NaN in the gap)."""

    def __init__(self, cid, route, m, n, k, w="f32", off=None, **kw):
        super().__init__(cid, route, m, n, k, xb=False, **kw)
        self.w, self.off = w, dict(off or {})
        self.fam = "skinny" if route.startswith("skinny") else "gemm_f32"
        self.tile = 16 if self.fam == "skinny" else 32           # the grid the tile figure is taken on
        self.step = 32 if self.fam == "skinny" else 16           # one K step of the kernel
        assert not (self.fam == "skinny" and w != "bf16")

    @property
    def klass(self):
        if self.fam == "skinny":
            return "skinny"
        return {"none": "plain", "silu": "silu"}.get(self.pro, "rms_mod" if self.mod else "rms")

    @property
    def data_key(self):      # everything the VALUES depend on: alignment offsets and the output pitch are not part of it
        return (self.fam, self.m, self.n, self.k, self.w, self.pro, bool(self.mod), self.bias, self.act,
                "row" if self.gate in ("n+4", "3n") else self.gate, bool(self.res), self.ldx)


def _cases():
    cs = []

    def add(cid, route, m, n, k, **kw):
        cs.append(FCase(cid, route, m, n, k, **kw))

    # ---- gemm_f32: the 64 x 64 tiles.  (n + 63) / 64 * (m + 63) / 64 >= 192: 897 x 961 is 15 x 16 = 240 tiles with one row and one column in
    # the last ones.  k = 48 (vec) and 50 (no float4 in K); bf16 weights at k = 48 are the matrix cores' (k % 16 == 0), so their vec case is k = 52
    for w in ("f32", "bf16"):
        kv = 48 if w == "f32" else 52
        add(f"g_{w}_t64_vec", _gemm(w, 0, 1, 64), 897, 961, kv, w=w, bias=True)
        add(f"g_{w}_t64_novec", _gemm(w, 0, 0, 64), 897, 961, 50, w=w, res="out")
        add(f"g_{w}_t64_dual_vec", _gemm(w, 1, 1, 64), 897, 961, kv, w=w, act="swiglu")
        add(f"g_{w}_t64_dual_novec", _gemm(w, 1, 0, 64), 897, 961, 50, w=w, act="swiglu", gate="chan")
    add("g_f32_t64_rms_dual", _gemm("f32", 1, 0, 64), 897, 961, 50, pro="rms", act="swiglu")      # rs[] of a 64-row tile with one row in it
    add("g_bf16_t64_rmsnow_mod", _gemm("bf16", 0, 1, 64), 897, 961, 52, w="bf16", pro="rms_now", mod="k+4", bias=True)
    # the threshold itself: 191 big tiles stay on 32 x 32, 192 take 64 x 64
    add("g_f32_191tiles", _gemm("f32", 0, 1, 32), 64, 12161, 20, bias=True)
    add("g_f32_192tiles", _gemm("f32", 0, 1, 64), 64, 12225, 20, bias=True)
    add("g_bf16_191tiles", _gemm("bf16", 0, 1, 32), 64, 12161, 20, w="bf16")
    add("g_bf16_192tiles", _gemm("bf16", 0, 1, 64), 64, 12225, 20, w="bf16")

    # ---- gemm_f32, 32 x 32 tiles: every M edge x every N edge, K slabs (TK = 16, float4 inside) and weight types taken in turn ----
    KS = {"f32": (7, 17, 20, 56, 224), "bf16": (7, 17, 20, 56, 1000)}      # bf16 weights at k % 16 == 0 belong to the matrix cores
    i = 0
    for m in (9, 17, 33, 65):
        for n in (1, 9, 31, 33, 70, 130):
            w = ("f32", "bf16")[i % 2]
            k = KS[w][(i // 2 + i // 6) % 5]
            add(f"g_{w}_m{m}_n{n}_k{k}", _gemm(w, 0, int(k % 4 == 0), 32), m, n, k, w=w, bias=bool(i % 3))
            i += 1
    add("g_f32_k1000", _gemm("f32", 0, 1, 32), 40, 96, 1000, bias=True)          # 63 slabs: the register prefetch handed over each round
    add("g_f32_k8960", _gemm("f32", 0, 1, 32), 40, 96, 8960, bias=True)          # the longest K the project uses
    add("g_f32_k8960_dual", _gemm("f32", 1, 1, 32), 17, 33, 8960, act="swiglu")
    add("g_bf16_k1000_dual", _gemm("bf16", 1, 1, 32), 40, 96, 1000, w="bf16", act="swiglu")

    # ---- every reason for vec = 0, one each, and the vec = 1 call they are one step away from ----
    for w in ("f32", "bf16"):
        add(f"g_{w}_vec", _gemm(w, 0, 1, 32), 33, 70, 56, w=w, bias=True)
        add(f"g_{w}_novec_k", _gemm(w, 0, 0, 32), 33, 70, 54, w=w, bias=True)                     # k % 4 != 0
        add(f"g_{w}_novec_ldx", _gemm(w, 0, 0, 32), 33, 70, 56, w=w, bias=True, ldx=57)           # ldx % 4 != 0
        add(f"g_{w}_novec_x4", _gemm(w, 0, 0, 32), 33, 70, 56, w=w, bias=True, off={"x": 1})      # x 4 bytes past a 16-byte boundary
        add(f"g_{w}_novec_w", _gemm(w, 0, 0, 32), 33, 70, 56, w=w, bias=True, off={"w": 1})       # w 4 (fp32) / 2 (bf16) bytes past one
        add(f"g_{w}_dual_vec", _gemm(w, 1, 1, 32), 33, 70, 56, w=w, act="swiglu")
        add(f"g_{w}_dual_novec_w2", _gemm(w, 1, 0, 32), 33, 70, 56, w=w, act="swiglu", off={"w2": 1})   # w2 misaligned, w aligned
        add(f"g_{w}_dual_novec_k", _gemm(w, 1, 0, 32), 33, 70, 17, w=w, act="swiglu")

    # ---- overlapping rows: the encoders' stem conv (k = 7, ldx = 1: rows overlap by 6 of 7, a partial first slab), the decoder's head conv
    # (n = 1), a transposed-conv view (ldx = cin, k = 2 cin, n = stride x cout) ----
    add("g_bf16_stem_3200x32x7", _gemm("bf16", 0, 0, 32), 3200, 32, 7, w="bf16", bias=True, ldx=1)
    add("g_f32_stem_3200x32x7", _gemm("f32", 0, 0, 32), 3200, 32, 7, bias=True, ldx=1)
    add("g_f32_head_3200x1x224", _gemm("f32", 0, 1, 32), 3200, 1, 224, bias=True, ldx=32)
    add("g_f32_convtr_40x120x48", _gemm("f32", 0, 1, 32), 40, 120, 48, bias=True, ldx=24)
    add("g_bf16_convtr_40x120x40", _gemm("bf16", 0, 1, 32), 40, 120, 40, w="bf16", bias=True, ldx=20)

    # ---- prologues, 33 rows (the second row tile holds one row: rs[] of rows >= M) ----
    for w in ("f32", "bf16"):
        add(f"g_{w}_rms", _gemm(w, 0, 1, 32), 33, 70, 56, w=w, pro="rms", bias=True)
        add(f"g_{w}_rmsnow", _gemm(w, 0, 0, 32), 33, 70, 17, w=w, pro="rms_now")
        add(f"g_{w}_rms_modk4", _gemm(w, 0, 1, 32), 33, 70, 56, w=w, pro="rms", mod="k+4")       # ld_mod = k + 4
        add(f"g_{w}_rmsnow_mod3k_rowgate", _gemm(w, 0, 1, 32), 33, 70, 56, w=w, pro="rms_now", mod="3k", gate="3n", res="inplace")
        add(f"g_{w}_silu", _gemm(w, 0, 1, 32), 33, 70, 56, w=w, pro="silu")
        add(f"g_{w}_silu_novec", _gemm(w, 0, 0, 32), 33, 70, 7, w=w, pro="silu", bias=True)
        add(f"g_{w}_rms_swiglu", _gemm(w, 1, 1, 32), 33, 70, 56, w=w, pro="rms", act="swiglu")
    add("g_f32_rms_k1000", _gemm("f32", 0, 1, 32), 40, 96, 1000, pro="rms", bias=True)
    add("g_bf16_rms_mod_k1000", _gemm("bf16", 0, 1, 32), 40, 96, 1000, w="bf16", pro="rms", mod="2k")

    # ---- epilogues ----
    E = [("gelu", dict(bias=True, act="gelu")), ("chan_gate", dict(gate="chan")), ("row_gate", dict(gate="n+4")), ("res", dict(res="out")),
         ("res_inplace", dict(bias=True, res="inplace")), ("res_ld1", dict(bias=True, res="out", scalar="ld")),                # ldo = ldres = n + 1
         ("gelu_gate_res_inplace_ld1", dict(bias=True, act="gelu", gate="n+4", res="inplace", scalar="ld")),
         ("swiglu_gate_res", dict(act="swiglu", gate="chan", res="out"))]
    for name, kw in E:
        for w in ("f32", "bf16"):
            add(f"g_{w}_{name}", _gemm(w, int(kw.get("act") == "swiglu"), 1, 32), 33, 70, 56, w=w, **kw)

    # ---- skinny: every K with ldx < k (a strided conv's view) and with ldx = k + 4 (NaN gaps); M at the route's bounds (5, 2048), in the
    # clamped last tile (17, 37), whole tiles (16) and many tiles (200, 1603); N 16, 48, 1280; bias present and absent ----
    def sk(cid, m, n, k, ldx, bias=True):
        add(cid, _skinny(*SKINNY_OF_K[k]), m, n, k, w="bf16", bias=bias, ldx=ldx)

    sk("s_k128_m1603_overlap", 1603, 32, 128, 64)
    sk("s_k128_m1603_gap", 1603, 32, 128, 132)               # the widest case of a streaming frame, three rows more
    sk("s_k128_m2048_gap", 2048, 16, 128, 132, bias=False)
    sk("s_k256_m5_overlap", 5, 48, 256, 128)
    sk("s_k256_m17_gap", 17, 16, 256, 260, bias=False)
    sk("s_k512_m37_overlap", 37, 48, 512, 256, bias=False)
    sk("s_k512_m200_gap", 200, 16, 512, 516)
    sk("s_k1024_m16_overlap", 16, 48, 1024, 512)
    sk("s_k1024_m17_gap", 17, 16, 1024, 1028, bias=False)
    sk("s_k2048_m37_overlap", 37, 16, 2048, 1024)
    sk("s_k2048_m5_gap", 5, 48, 2048, 2052, bias=False)
    sk("s_k2560_m17_overlap", 17, 48, 2560, 1024)            # k / 10 * 4: a stride-4 view of 10 taps
    sk("s_k2560_m16_gap", 16, 16, 2560, 2564, bias=False)
    sk("s_k5120_m37_overlap", 37, 48, 5120, 2560, bias=False)
    sk("s_k5120_m5_gap", 5, 16, 5120, 5124)
    # the resampling convs of one streaming frame as decoder_run / encoder_run form them (test_production_shapes_have_cases)
    sk("s_dec_8x2560x2048", 8, 2560, 2048, 1024)
    sk("s_dec_40x1280x1024", 40, 1280, 1024, 512)
    sk("s_dec_200x512x512", 200, 512, 512, 256)
    sk("s_frame_800x128x256", 800, 128, 256, 128)
    sk("s_frame_1600x64x128", 1600, 64, 128, 64)
    sk("s_enc_200x256x1024", 200, 256, 1024, 512)
    sk("s_enc_40x512x2560", 40, 512, 2560, 1280)
    sk("s_enc_8x1024x5120", 8, 1024, 5120, 2560)
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
# fixed shapes (m, n, k, ldx, wdt) whose default routes a leaked vv_tune("skinny") would change, and one of the other family
HYGIENE = [((40, 512, 2560, 1280, "bf16"), _skinny(20, 1)), ((1603, 32, 128, 64, "bf16"), _skinny(1, 1)), ((33, 70, 56, 56, "bf16"), _gemm("bf16", 0, 1, 32))]


def instantiation_table():
    lines = []
    for inst in ALL_INSTANTIATIONS:
        ids = [c.id for c in CASES if c.route == inst]
        text = ", ".join(ids[:4]) + (f", ... ({len(ids)} cases)" if len(ids) > 4 else "")
        lines.append(f"  {inst:<42} {text}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# operands, the fp64 reference and the fp32 stand-ins (CPU)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands_of(key):
    fam, m, n, k, w, pro, mod, bias, act, gate, res, ldx = key
    g = torch.Generator().manual_seed(zlib.crc32(repr((fam, m, n, k, w, pro, act, ldx or 0)).encode()))
    o = {}
    if ldx and ldx < k:                          # overlapping rows: one flat buffer, row r starts at r * ldx
        flat = torch.randn((m - 1) * ldx + k, generator=g)
        o["x_flat"], o["x"] = flat, flat.as_strided((m, k), (ldx, 1))
    elif ldx:                                    # a pitch of the case's own: NaN between the rows
        x = torch.randn(m, k, generator=g)
        flat = torch.full(((m - 1) * ldx + k,), NAN)
        flat.as_strided((m, k), (ldx, 1)).copy_(x)
        o["x_flat"], o["x"] = flat, x
    else:
        o["x"] = torch.randn(m, k, generator=g)
    cast = (lambda t: t) if w == "f32" else (lambda t: t.bfloat16())
    o["w"] = cast(torch.randn(n, k, generator=g) / k ** 0.5)
    if act == "swiglu":
        o["w2"] = cast(torch.randn(n, k, generator=g) / k ** 0.5)
    if pro == "rms":
        o["norm_w"] = 1 + 0.1 * torch.randn(k, generator=g)
    if mod:
        o["shift"], o["scale"] = 0.2 * torch.randn(m, k, generator=g), 0.2 * torch.randn(m, k, generator=g)
    if bias:
        o["bias"] = 0.1 * torch.randn(n, generator=g)
    if gate == "chan":
        o["gate"] = torch.randn(n, generator=g)
    elif gate == "row":
        o["gate"] = torch.randn(m, n, generator=g)
    if res:
        o["res"] = torch.randn(m, n, generator=g)
    return o


def operands(case):
    return _operands_of(case.data_key)


def reference(case, o=None):
    """fp64 on the operands as the device receives them: gemm_f32 rounds nothing, skinny rounds x to bf16 once"""
    return ref_linear_fp64(operands(case) if o is None else o, case.pro, case.act, False, False, round_act=case.fam == "skinny")


def chain_f32(xh, w, skip=None, rs=slice(None), cs=slice(None)):
    """gemm_kernel's accumulation: per output ONE ascending chain of fp32 fused multiply-adds over k (a product of two fp32 values is exact in
    fp64, and the sum is rounded to fp32 once per link).  skip: a 16-wide K step left out."""
    xd, wd = xh[rs].double(), w[cs].double().t().contiguous()
    acc = torch.zeros(xd.shape[0], wd.shape[1])
    for kk in range(xd.shape[1]):
        if skip is None or not (16 * skip <= kk < 16 * skip + 16):
            acc = (acc.double() + xd[:, kk: kk + 1] * wd[kk: kk + 1, :]).float()
    return acc


def waves_f32(xb, w, skip=None, rs=slice(None), cs=slice(None), row_of=None):
    """skinny_kernel's accumulation: K in 32-wide steps, a quarter of them per wave accumulated in fp32, the four partial sums added in wave
    order.  skip: one step left out.  row_of: the input row each output row is computed from (a wrong kernel's, for the tests of the figures)"""
    xs = xb[rs].contiguous() if row_of is None else xb[row_of].contiguous()
    ws = w[cs].float()
    (m, k), n = xs.shape, ws.shape[0]
    S = k // 32
    P = torch.bmm(xs.reshape(m, S, 32).transpose(0, 1), ws.reshape(n, S, 32).permute(1, 2, 0))
    total = None
    for wave in range(4):
        acc = torch.zeros(m, n)
        for s in range(wave * S // 4, (wave + 1) * S // 4):
            if s != skip:
                acc = acc + P[s]
        total = acc if total is None else total + acc
    return total


def figures(case, got, ref):
    """(global, worst tile, worst row or 0.0 where a row has fewer than ROW_MIN_COLS columns), (tile index, row index)"""
    t, ti, r, ri = tile_row_errors(got, ref, case.tile, case.tile)
    return (_rel(got, ref), t, r if case.n >= ROW_MIN_COLS else 0.0), (ti, ri)


def _drop_steps(case):
    S = -(-case.k // case.step)
    return sorted({0, S // 2, S - 1})


def stand_in(case, o, skip=None, tile=(0, 0), row_of=None):
    """The fp32 restatement of the case (fp64 result): whole output, or - skip given - tile `tile` alone with K step `skip` left out"""
    T = case.tile
    rs = slice(None) if skip is None else slice(tile[0] * T, min(tile[0] * T + T, case.m))
    cs = slice(None) if skip is None else slice(tile[1] * T, min(tile[1] * T + T, case.n))
    if case.fam == "skinny":
        y, y2 = waves_f32(o["x"].bfloat16().float(), o["w"], skip, rs, cs, row_of), None
    else:
        xh = _prologue(o["x"], o, case.pro, torch.float32)
        y = chain_f32(xh, o["w"], skip, rs, cs)
        y2 = chain_f32(xh, o["w2"], skip, rs, cs) if "w2" in o else None
    return _epilogue(y, y2, o, case.act, torch.float32, rs, cs).double(), rs, cs


@functools.lru_cache(maxsize=None)
def _expect_of(cid):
    """(fp64 reference, floor (global, tile, row) of the fp32 stand-in, cost of one dropped K step in the tile it is dropped from) - cached per
    set of operands through the case that owns them"""
    case = CASES[CASE_IDS.index(cid)]
    o = operands(case)
    ref = reference(case)
    floor = figures(case, stand_in(case, o)[0].numpy(), ref.numpy())[0]
    drop = math.inf
    for s0 in _drop_steps(case):                 # the first tile; the cheapest of the first, middle and last step
        y, rs, cs = stand_in(case, o, skip=s0)
        drop = min(drop, _rel(y.numpy(), ref[rs, cs].numpy()))
    return ref, floor, drop


_OWNER = {}
for _c in CASES:
    _OWNER.setdefault(_c.data_key, _c.id)


def expect(case):
    return _expect_of(_OWNER[case.data_key])


# ---------------------------------------------------------------------------------------------------------------
# CPU-only guards
# ---------------------------------------------------------------------------------------------------------------
def test_overlapping_rows_are_the_convs():
    """Guards the "rows may overlap" reading of the reference (CPU only).  A strided conv and a transposed conv as decoder_run / encoder_run of
    csrc/vv_model.hip hand them to vv_linear - rows of pitch stride x cin (cin) over the padded channels-last input, the weight layouts of
    Weights._conv: [co, (tap, ci)], and [(r, co), (j, ci)] with the tap flip - against torch's conv1d / conv_transpose1d in fp64, for the
    unrounded (gemm_f32) and the bf16-rounded (skinny) reference."""
    F = torch.nn.functional
    g = torch.Generator().manual_seed(11)
    # strided: kk taps, stride s, Tout outputs over a padded input of (Tout - 1) s + kk rows
    cin, cout, kk, s, Tout = 4, 6, 4, 2, 9
    rows = (Tout - 1) * s + kk
    flat = torch.randn(rows * cin, generator=g)
    w, b = torch.randn(cout, cin, kk, generator=g), torch.randn(cout, generator=g)
    o = {"x": flat.as_strided((Tout, kk * cin), (s * cin, 1)), "w": w.permute(0, 2, 1).reshape(cout, kk * cin), "bias": b}
    for rounded in (False, True):
        xin = bf16_round64(flat) if rounded else flat.double()
        want = F.conv1d(xin.view(rows, cin).t()[None], w.double(), b.double(), stride=s)[0].t()
        got = ref_linear_fp64(o, round_act=rounded)
        assert got.shape == want.shape == (Tout, cout) and _rel(got.numpy(), want.numpy()) < 1e-12
    # transposed, kernel 2 s: row t of the view is [x[t - 1], x[t]] (one context row in front), output row t holds times t s .. t s + s - 1
    cin, cout, s, T = 4, 3, 5, 7
    flat = torch.randn((T + 1) * cin, generator=g)
    w, b = torch.randn(cin, cout, 2 * s, generator=g), torch.randn(cout, generator=g)
    wl = w.reshape(cin, cout, 2, s).flip(2).permute(3, 1, 2, 0).reshape(s * cout, 2 * cin)       # [(r, co), (j, ci)]: j = 0 -> taps r + s
    o = {"x": flat.as_strided((T, 2 * cin), (cin, 1)), "w": wl, "bias": b.repeat(s)}
    for rounded in (False, True):
        xin = bf16_round64(flat) if rounded else flat.double()
        full = F.conv_transpose1d(xin.view(T + 1, cin).t()[None], w.double(), b.double(), stride=s)[0].t()     # [(T + 2) s, cout]
        want = full[s: s + T * s]                                      # the times the T new inputs complete
        got = ref_linear_fp64(o, round_act=rounded).reshape(T * s, cout)
        assert _rel(got.numpy(), want.numpy()) < 1e-12


def test_operands_with_a_pitch_of_their_own():
    """ldx >= k leaves NaN between the rows and the strided view of the flat buffer is the case's x; ldx < k rows share their elements"""
    gap = CASES[CASE_IDS.index("s_k256_m17_gap")]
    o = operands(gap)
    assert torch.equal(o["x_flat"].as_strided((gap.m, gap.k), (gap.ldx, 1)), o["x"]) and int(torch.isnan(o["x_flat"]).sum()) == (gap.m - 1) * 4
    lap = CASES[CASE_IDS.index("g_bf16_stem_3200x32x7")]
    o = operands(lap)
    assert o["x_flat"].numel() == 3199 + 7 and torch.equal(o["x"][5, 1:], o["x"][6, :-1])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_step(cid):
    """Both conditions on the class bar, for every case (CPU only): at least 8 x the fp32 stand-in's own error against the fp64 reference
    (global, worst tile, worst row where n >= 8), at most a tenth of what one dropped K step (16 wide for gemm_f32, 32 wide for skinny) costs
    the tile it is dropped from."""
    case = CASES[CASE_IDS.index(cid)]
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} tile {floor[1]:.2e} row {floor[2]:.2e}  dropped step {drop:.2e}")
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


def test_wrong_stand_ins_miss_the_bar():
    """The figures see what they are for (CPU only).  A K step dropped in ONE tile in the middle of a many-tile output stays under the bar in the
    global figure and misses it in the tile figure; a skinny last tile whose row M - 1 is read from row M - 2 misses it in the tile and the row."""
    case = next(c for c in CASES if c.fam == "gemm_f32" and c.m == 65 and c.n == 130)
    o, ref = operands(case), expect(case)[0]
    good = stand_in(case, o)[0].clone()
    y, rs, cs = stand_in(case, o, skip=0, tile=(1, 2))
    good[rs, cs] = y
    (g, t, r), (ti, _) = figures(case, good.numpy(), ref.numpy())
    assert ti == (1, 2) and t > BAR[case.klass], (g, t, r, ti)
    big = CASES[CASE_IDS.index("s_k128_m1603_overlap")]
    o, ref = operands(big), expect(big)[0]
    good = stand_in(big, o)[0].clone()
    y, rs, cs = stand_in(big, o, skip=1, tile=(50, 1))
    good[rs, cs] = y
    (g, t, r), (ti, _) = figures(big, good.numpy(), ref.numpy())
    assert ti == (50, 1) and t > BAR["skinny"] and g < 0.1 * t, (g, t, r, ti)
    clamp = CASES[CASE_IDS.index("s_k512_m37_overlap")]
    o, ref = operands(clamp), expect(clamp)[0]
    rows = torch.arange(clamp.m).clamp(max=clamp.m - 2)                 # min(t, M - 2) where the kernel has min(t, M - 1)
    wrong = _epilogue(waves_f32(o["x"].bfloat16().float(), o["w"], row_of=rows), None, o, "none", torch.float32).double()
    (g, t, r), (ti, ri) = figures(clamp, wrong.numpy(), ref.numpy())
    assert ri == clamp.m - 1 and ti[0] == 2 and r > BAR["skinny"] and t > BAR["skinny"], (g, t, r, ti, ri)


def test_docstring_table_is_current():
    """the instantiation -> case table of the docstring is the one the parametrisation generates, and names all 16 + 7 instantiations"""
    assert instantiation_table() in __doc__
    routes = {c.route for c in CASES}
    assert routes == set(ALL_INSTANTIATIONS) and len(ALL_INSTANTIATIONS) == 23, routes ^ set(ALL_INSTANTIATIONS)


def test_every_listed_edge_has_a_case():
    """the M, N and K edges, the route's bounds and both bias forms are all among the cases"""
    gm = [c for c in CASES if c.fam == "gemm_f32"]
    sk = [c for c in CASES if c.fam == "skinny"]
    assert {9, 17, 33, 65} <= {c.m for c in gm} and {1, 9, 31, 33, 70, 130} <= {c.n for c in gm}
    assert {7, 17, 20, 56, 224, 1000, 8960} <= {c.k for c in gm}
    assert {5, 16, 17, 37, 200, 1603, 2048} <= {c.m for c in sk} and {16, 48, 1280} <= {c.n for c in sk}
    for k in SKINNY_OF_K:
        assert any(c.k == k and c.ldx < k for c in sk) and any(c.k == k and c.ldx == k + 4 for c in sk), k
    assert {c.bias for c in sk} == {True, False}
    assert {c.klass for c in CASES} == set(BAR)


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """The code objects of vv_kernels.hip and vv_convffn.hip hold the 16 instantiations of gemm_kernel and the 7 of skinny_kernel and no other
    (CPU only: symbol names of the object files build() left)"""
    def gemm_name(w, dual, vec, tm, tn):
        assert tm == tn
        return _gemm(w, dual, vec, tm)

    got = instantiations_of(built_kernels("vv_kernels.hip", tmp_path), {"gemm_kernel": gemm_name})
    got |= instantiations_of(built_kernels("vv_convffn.hip", tmp_path), {"skinny_kernel": _skinny})
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))


# ---------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------
def lay_out(case):
    """layout() of tests/test_hip_mfma_gemm.py, then the operands of case.off moved that many elements past their allocation's start (NaN in
    front): {name: host image}, {field: stride}"""
    buf, ld = layout(case, operands(case))
    for name, e in case.off.items():
        t = buf[name].reshape(-1)
        buf[name] = torch.cat([torch.full((e,), NAN, dtype=t.dtype), t])
    return buf, ld


def args_of(case, ld, ptr):
    """vv_lin_args of the case; ptr: {name: address of the allocation lay_out() describes}"""
    L = _lib()[0]
    p = dict(ptr)
    for name, e in case.off.items():
        p[name] += e * (4 if name == "x" or case.w == "f32" else 2)
    a = fill_args(case, ld, p)
    a.wdt = L.VV_F32 if case.w == "f32" else L.VV_BF16
    return a


def plain_args(m, n, k, ldx, w="bf16", bias=True):
    """a conv's call as csrc/vv_model.hip forms it: x, w, bias, out with ldo = n; stand-in addresses"""
    L = _lib()[0]
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo = _FAKE["x"], ldx, m, n, k, L.VV_F32 if w == "f32" else L.VV_BF16, _FAKE["w"], _FAKE["out"], n
    if bias:
        a.bias = _FAKE["bias"]
    return a


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_case_on_the_host(cid):
    """The route query needs no device: every case's arguments (stand-in addresses, nothing is dereferenced) report the instantiation the case is
    named for, here on the CPU too."""
    case = CASES[CASE_IDS.index(cid)]
    got = route_of(args_of(case, lay_out(case)[1], _FAKE))
    assert got == case.route, (cid, got, case.route)


def test_skinny_route_boundaries():
    """CPU only.  One step outside what skinny_kernel covers takes another named route: too few and too many rows, a K without an instantiation,
    n % 16, a pitch or an address the float4 loads cannot take, and every epilogue or prologue the kernel does not have."""
    L = _lib()[0]

    def route(m=40, n=512, k=512, ldx=256, **kw):
        a = plain_args(m, n, k, ldx)
        for f, v in kw.items():
            setattr(a, f, v)
        return route_of(a)

    mfma = "mfma_stream<dual=0,ksplit=1,xb=0,mt=1>"
    assert route() == _skinny(4, 1) and route(m=5) == _skinny(4, 1) and route(m=2048) == _skinny(4, 1)
    assert route(m=4).startswith("gemv_stream<m=4,"), route(m=4)
    assert route(m=2049) == mfma
    assert route(k=384, ldx=192) == mfma
    assert route(n=24) == mfma
    assert route(ldx=510) == _gemm("bf16", 0, 0, 32)                   # ldx % 4 != 0: the matrix-core path declines it too
    assert route(x=_FAKE["x"] + 4) == _gemm("bf16", 0, 0, 32)          # x 4 bytes past a 16-byte boundary
    assert route(res=_FAKE["res"], ldres=512) == mfma
    assert route(gate=_FAKE["gate"]) == mfma
    assert route(pro=L.PRO_SILU) == mfma
    assert route(pro=L.PRO_RMSNORM, norm_w=_FAKE["norm_w"]) == mfma
    assert route(act=L.ACT_GELU) == mfma
    assert route(act=L.ACT_SWIGLU, w2=_FAKE["w2"]) == "mfma_stream<dual=1,ksplit=1,xb=0,mt=1>"


def test_skinny_switched_off_takes_the_matrix_core_stream():
    """vv_tune("skinny", 0) sends the same arguments to mfma_stream<...>; switched back on, they are the skinny kernel's again (CPU only)"""
    L, l = _lib()[:2]
    try:
        L.check(l.vv_tune(b"skinny", 0), "vv_tune")
        for (m, n, k, ldx, w), _ in HYGIENE[:2]:
            assert route_of(plain_args(m, n, k, ldx, w)) == "mfma_stream<dual=0,ksplit=1,xb=0,mt=1>"
    finally:
        L.check(l.vv_tune(b"skinny", 1), "vv_tune")
    for (m, n, k, ldx, w), want in HYGIENE:
        assert route_of(plain_args(m, n, k, ldx, w)) == want


def frame_calls(cfg):
    """(who, m, n, k, ldx) of every vv_linear call the stem, resampling and head convs make in one streaming frame - T0 = 1 for the decoder, one
    hop of samples for the two encoders - as decoder_run / encoder_run of csrc/vv_model.hip form them: a strided conv (Tout, cout, kk cin,
    ldx = stride cin), a transposed one (T, stride cout, 2 cin, ldx = cin).  Channel counts and kernels: vibevoice_rocm_amd/synth.py."""
    calls = []
    n = len(cfg.ac_depths)
    T, c = 1, cfg.ac_dec_filters * 2 ** (n - 1)
    calls.append(("ac_dec.stem", T, c, 7 * cfg.ac_dim, cfg.ac_dim))
    for i in range(1, n):
        c, s = cfg.ac_dec_filters * 2 ** (n - 1 - i), cfg.ac_ratios[i - 1]
        calls.append((f"ac_dec.up{i}", T, s * c, 2 * (2 * c), 2 * c))
        T *= s
    calls.append(("ac_dec.head", T, 1, 7 * c, c))
    assert T == cfg.hop
    for who, filt, ratios, depths, dim in (("ac_enc", cfg.ac_filters, cfg.ac_ratios, cfg.ac_depths, cfg.ac_dim),
                                           ("sem_enc", cfg.sem_filters, cfg.sem_ratios, cfg.sem_depths, cfg.sem_dim)):
        rr, T = list(reversed(ratios)), cfg.hop
        calls.append((who + ".stem", T, filt, 7, 1))
        for i in range(1, len(depths)):
            c, s = filt * 2 ** i, rr[i - 1]
            T //= s
            calls.append((f"{who}.down{i}", T, c, 2 * s * (c // 2), s * (c // 2)))
        calls.append((who + ".head", T, dim, 7 * c, c))
        assert T == 1
    return calls


@pytest.mark.parametrize("preset", ["1.5b", "7b"])
def test_production_shapes_have_cases(preset):
    """CPU only.  Every conv call of one streaming frame that routes to skinny<...> or gemm_f32<...>, on bf16 and on fp32 weights, lands on an
    instantiation that has a parity case; the bf16 encoder stem and every skinny call are cases shape for shape."""
    from vibevoice_rocm_amd.config import VVConfig
    covered = {c.route for c in CASES}
    shapes = {(c.m, c.n, c.k, c.ldx, c.w) for c in CASES if c.bias and not c.off and c.pro == "none" and c.act == "none" and not c.gate and not c.res}
    seen = {"skinny": 0, "gemm_f32": 0}
    for who, m, n, k, ldx in frame_calls(VVConfig.preset(preset)):
        for w in ("bf16", "f32"):
            r = route_of(plain_args(m, n, k, ldx, w))
            fam = r.split("<")[0]
            print(f"{preset} {who:<14} {w:<4} m {m:>4} n {n:>4} k {k:>5} ldx {ldx:>4}  {r}")
            if fam not in seen:
                continue
            seen[fam] += 1
            assert r in covered, (who, w, r)
            if fam == "skinny" or (who.endswith("enc.stem") and w == "bf16"):
                assert (m, n, k, ldx, w) in shapes, (who, m, n, k, ldx, w, r)
            if who.endswith("enc.stem"):
                assert (m, n, k, ldx) == (3200, 32, 7, 1) and r == _gemm(w, 0, 0, 32), (who, r)
    assert seen["skinny"] >= 10 and seen["gemm_f32"] >= 10, seen      # 5 + 5 resampling convs on bf16; every m > 8 conv on fp32


_MEASURED = {}      # class -> [global, tile, row] maxima of this session, written by _report


def run_case(case):
    """Lay the case out, assert its route, launch it twice into separate outputs; returns out[m, n] as fp64"""
    L, l = _lib()[:2]
    buf, ld = lay_out(case)
    m, n, ldo, off = case.m, case.n, ld["ldo"], ld["out_off"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda(), buf["out"].cuda()]
    for out in outs:
        a = args_of(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
        got_route = route_of(a)
        assert got_route == case.route, (case.id, got_route, case.route)
        L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    h0, h1 = outs[0].cpu(), outs[1].cpu()
    assert _same_bits(h0, h1), f"{case.id}: two runs of the same call differ"
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    grid = h0[off:].view(m + 2, ldo)
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    assert torch.isfinite(grid[inside]).all(), f"{case.id}: {int((~torch.isfinite(grid[inside])).sum())} in-range outputs are not finite"
    assert torch.isnan(grid[~inside]).all() and torch.isnan(h0[:off]).all(), f"{case.id}: a gap or guard element of out was written"
    return grid[:m, :n].double()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemm_f32_and_skinny_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref, floor, drop = expect(case)
    got = run_case(case).numpy()
    rel_rms(got, ref.numpy(), f"{cid} [{case.route}] global")
    (g, t, r), (ti, ri) = figures(case, got, ref.numpy())
    bar, T = BAR[case.klass], case.tile
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst tile {t:.3e} at (row tile {ti[0]}, channel tile {ti[1]})  "
          f"worst row {r:.3e} (row {ri}{'' if case.n >= ROW_MIN_COLS else ': not taken, n < 8'})  [floor {max(floor):.2e}, dropped step {drop:.2e}]")
    mx = _MEASURED.setdefault(case.klass, [0.0, 0.0, 0.0])
    for i, v in enumerate((g, t, r)):
        mx[i] = max(mx[i], v)
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert t < bar, f"{cid}: {T} x {T} tile (row tile {ti[0]}, channel tile {ti[1]}) rel RMS {t:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"


@pytest.mark.gpu
def test_zz_skinny_switch_is_back_at_its_default():
    """Hook hygiene: fixed shapes report their default routes, so a vv_tune("skinny") setting leaked by a test above fails here."""
    _need_gpu()
    for (m, n, k, ldx, w), want in HYGIENE:
        assert route_of(plain_args(m, n, k, ldx, w)) == want
    _report()


def _report():
    """the session's largest figures per class, for the docstring and profiles/gemm_f32_skinny_parity.txt (written only where
    VV_GEMM_F32_PARITY_OUT says)"""
    path = os.environ.get("VV_GEMM_F32_PARITY_OUT")
    if not path or not _MEASURED:
        return
    with open(path, "w") as f:
        f.write(f"{torch.cuda.get_device_name(0)}: largest rel RMS against fp64 over each class's cases (tests/test_hip_gemm_f32.py)\n")
        f.write(f"{'class':<9} {'cases':>5} {'bar':>8} {'global':>10} {'tile':>10} {'row':>10} {'bar / largest':>14}\n")
        for k in BAR:
            if k in _MEASURED:
                g, t, r = _MEASURED[k]
                f.write(f"{k:<9} {sum(c.klass == k for c in CASES):>5} {BAR[k]:>8.1e} {g:>10.2e} {t:>10.2e} {r:>10.2e} {BAR[k] / max(g, t, r):>14.1f}\n")


if __name__ == "__main__":
    if "--table" in sys.argv:
        print(instantiation_table())

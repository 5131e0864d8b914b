"""Every matrix-core GEMM kernel of vv_mfma_gemm.hip against one fp64 reference, per output tile - through the C ABI only, no engine, no weights.

Each case first asks `vv_linear_route` which kernel its arguments take and asserts the instantiation it means to test; the 30 instantiations
(24 of mfma_linear_kernel<dual, ksplit, xb, mt>, 6 of mfma_tiled_kernel<dual, bk, tm>) are each reached by at least one case (table below).

The reference (`ref_linear_fp64`) is plain torch fp64 on the operands as the device received them and knows nothing of tiles: a bf16 x is widened
exactly, an fp32 x takes its prologue in fp64 and is rounded to bf16 once (as the kernel documents), the product and the epilogue are fp64, a bf16
output is rounded once.  Three figures per case: global rel RMS, the worst aligned 32 x 32 output tile (edge tiles cut at M and N) and the worst row.

Bars: one constant per route class (BAR).  `test_bars_sit_between_floor_and_dropped_step` (CPU) holds every case to both conditions:
  bar >= 8 x the case's floor - the error of a torch fp32 stand-in of the same operation (fp32 prologue, rounded where the kernel rounds,
         accumulated in 16-wide K steps) against the fp64 reference; the factor is headroom for another summation order and rsqrtf / expf;
  bar <= 1/10 of what one dropped 16-wide K step in one tile costs that tile (measured by removing the step from the stand-in).
How each constant was chosen is written at BAR.

Every case lays its operands out with NaN in every pitch gap (ldx = k + 8, ldo = ldres = n + 4, ...) and two NaN guard rows behind the output,
runs twice into separate buffers (bit-identical: the K-split combine has a fixed order), and checks that every in-range output is finite, every
gap and guard is still NaN and every input is bit-unchanged.

Measured on the MI355X, largest value over the class's cases, global / worst tile / worst row rel RMS against fp64 (profiles/mfma_gemm_parity.txt):
  class     cases   bar      global / tile / row              bar / largest
  xb           57   1e-4     5.9e-7 / 1.0e-6 / 7.7e-7              99
  none         11   1e-4     7.1e-8 / 7.4e-8 / 9.5e-8            1049
  rms          16   6e-3     2.8e-5 / 1.0e-4 / 3.3e-4              18
  rms_mod      10   5e-3     3.0e-5 / 6.8e-5 / 1.7e-4              29
  silu          5   5e-3     1.0e-7 / 1.4e-7 / 1.3e-7           36600
  bf16         11   6e-3     1.1e-5 / 9.8e-5 / 1.2e-4              51
No value is within a factor of ten of its bar.  The nearest, 3.3e-4 for one row of the unhooked MT = 2 staged kernel (RMSNorm + SwiGLU, K = 1040), is
one activation whose bf16 rounding the device's fp32 prologue flips against the fp64 one: 18 times below 6e-3.  vv_cast_rows_bf16: VV_PRO_NONE
bit-exact, RMSNorm within one bf16 ulp with at most 4.3e-5 of a case's elements differing (cap 1e-3).

Instantiation -> case ids (generated: `python tests/test_hip_mfma_gemm.py --table`; `test_docstring_table_is_current` keeps it so):
  mfma_stream<dual=0,ksplit=0,xb=1,mt=1>     s_l_k128_bias_rows0, s_l_k128_gate_res_rows0, s_s_k32_rows0, s_s_k96_rows0, ... (11 cases)
  mfma_stream<dual=1,ksplit=0,xb=1,mt=1>     s_d64_k192_rows0, s_d64_k192_bf16out_rows0, s_d32q_k96_rows0, s_d32q_k352_rows0, ... (6 cases)
  mfma_stream<dual=0,ksplit=1,xb=1,mt=1>     s_l_k640_rows0, s_l_k640_gelu_bf16out_rows0, s_narrow_64x64_rows0, s_narrow_70x192_bias_rows0, ... (11 cases)
  mfma_stream<dual=1,ksplit=1,xb=1,mt=1>     s_d64_k576_rows0, x_ks1_dual, x_ks1_dual_bf16out
  mfma_stream<dual=0,ksplit=0,xb=1,mt=2>     x_mt2_ks0_hook
  mfma_stream<dual=1,ksplit=0,xb=1,mt=2>     x_mt2_ks0_dual_hook
  mfma_stream<dual=0,ksplit=1,xb=1,mt=2>     x_mt2_ks1_hook
  mfma_stream<dual=1,ksplit=1,xb=1,mt=2>     x_mt2_ks1_dual_hook
  mfma_stream<dual=0,ksplit=0,xb=1,mt=4>     x_mt4_ks0_hook
  mfma_stream<dual=1,ksplit=0,xb=1,mt=4>     x_mt4_ks0_dual_hook
  mfma_stream<dual=0,ksplit=1,xb=1,mt=4>     s_q_k1024_bias_res_rows0, s_q_k1152_bias_res_inplace_rows0, x_mt4_plain
  mfma_stream<dual=1,ksplit=1,xb=1,mt=4>     x_mt4_dual
  mfma_stream<dual=0,ksplit=0,xb=0,mt=1>     f_none_bias_res_ks0, f_none_bias_res_ks0_scalar, f_rms_bias_ks0, f_rms_bias_ks0_scalar, ... (14 cases)
  mfma_stream<dual=1,ksplit=0,xb=0,mt=1>     f_rms_swiglu_ks0, f_rms_swiglu_ks0_scalar
  mfma_stream<dual=0,ksplit=1,xb=0,mt=1>     f_none_bias_res_ks1, f_none_bias_res_ks1_scalar, f_rms_bias_ks1, f_rms_bias_ks1_scalar, ... (20 cases)
  mfma_stream<dual=1,ksplit=1,xb=0,mt=1>     f_rms_swiglu_ks1, f_rms_swiglu_ks1_scalar
  mfma_stream<dual=0,ksplit=0,xb=0,mt=2>     f_mt2_ks0_hook
  mfma_stream<dual=1,ksplit=0,xb=0,mt=2>     f_mt2_ks0_dual_hook
  mfma_stream<dual=0,ksplit=1,xb=0,mt=2>     f_mt2_rms_bias
  mfma_stream<dual=1,ksplit=1,xb=0,mt=2>     f_mt2_rms_swiglu
  mfma_stream<dual=0,ksplit=0,xb=0,mt=4>     f_mt4_ks0_hook
  mfma_stream<dual=1,ksplit=0,xb=0,mt=4>     f_mt4_ks0_dual_hook
  mfma_stream<dual=0,ksplit=1,xb=0,mt=4>     f_mt4_k528_hook
  mfma_stream<dual=1,ksplit=1,xb=0,mt=4>     f_mt4_k528_dual_hook
  mfma_tiled<dual=1,bk=64,tm=64>             t_d64_k192, t_d64_k576, t_d64_k192_bf16out
  mfma_tiled<dual=1,bk=32,tm=64>             t_d32q_k96, t_d32q_k352, t_dualbk64off_k192
  mfma_tiled<dual=0,bk=128,tm=64>            t_q_k1024_bias_res, t_q_k1152_bias_res_inplace, t_narrow_64x64, t_narrow_70x192_bias
  mfma_tiled<dual=0,bk=128,tm=128>           t_l_k128_bias, t_l_k640, t_l_k640_gelu_bf16out, t_l_k128_gate_res, ... (6 cases)
  mfma_tiled<dual=0,bk=32,tm=128>            t_s_k32, t_s_k96, t_s_k288, t_s_k224_overlap, ... (5 cases)
  mfma_tiled<dual=1,bk=32,tm=128>            t_dbig_k96_hook, t_dbig_256tiles
"""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import rel_rms

EPS = 1e-5

# One constant per route class, held for the global, the worst-tile and the worst-row figure alike.  Chosen from the arithmetic, then checked
# against both conditions on the CPU (test_bars_sit_between_floor_and_dropped_step); never from what the device gives.
#   xb       bf16 operands are exact in the reference, so the error is fp32 accumulation alone: <= sqrt(K) 2^-24 of the sum's own rms for a
#            random-sign sum, 5e-6 at the longest K here (8208); a single-column or single-row edge tile divides by a few reference values that can
#            be ~ 10x below rms, so 1e-4.  The cheapest dropped step here (K = 8192: sqrt(16 / 8192) = 4.4e-2) is 400x above it.
#   none     fp32 x, no prologue: rounding to bf16 is the same operation in the reference and on the device, so the class behaves like xb.
#   rms      the prologue's fp32 rounding flips the bf16 rounding of ~ 2e-5 of the activations, and the device (rsqrtf, another summation
#            order of the mean) flips others than torch does.  One flipped activation x_j moves every output of its row by 2^-8 |x_j w_nj|:
#            against a row rms of ~ |x|_rms that is 2^-8 (|x_j| / |x|_rms) / sqrt(K) - 1.2e-3 for a 3-sigma activation at K = 96, the shortest
#            here, and up to twice that through SwiGLU, where both factors move: 2.4e-3 for the worst row.  6e-3 leaves a second flip in the
#            same row room; the cheapest dropped step of the class (K = 1040) costs its tile 1.1e-1.
#   rms_mod  the same with two more fp32 operations (x (1 + scale) + shift) in front of the rounding, no SwiGLU in the class, but K up to
#            2064, where a dropped step costs 5.8e-2: 5e-3.
#   silu     the same with expf and a division in front of the rounding: 5e-3 (cheapest dropped step 1.3e-1 at K = 1040).
#   bf16     one bf16 ulp (2^-8 relative) on the few outputs whose rounding flips: a flip on the largest element of a one-row edge tile
#            (32 values, peak / rms ~ 2.5) costs 2^-8 x 2.5 / sqrt(32) = 1.7e-3, two flips in one such tile 2.5e-3, and a staged prologue adds
#            its own flips.  6e-3; K <= 640 in this class, so a dropped step costs >= sqrt(16 / 640) = 1.6e-1 before the activation.
BAR = {"xb": 1e-4, "none": 1e-4, "rms": 6e-3, "rms_mod": 5e-3, "silu": 5e-3, "bf16": 6e-3}
FLOOR_HEADROOM = 8.0
DROP_MARGIN = 10.0
CAST_FLIP_CAP = 1e-3       # share of RMSNorm-cast elements that may differ from the fp64 reference at all (each by one bf16 ulp)

TUNE_DEFAULTS = {"mfma_mt": 0, "mfma_tiled_rows": 32, "mfma_tiled_bk128": 1, "mfma_tiled_small": 200, "mfma_tiled_dual_bk64": 1,
                 "mfma_tiled_small_dual": 256}


def _stream(dual, ksplit, xb, mt):
    return f"mfma_stream<dual={dual},ksplit={ksplit},xb={xb},mt={mt}>"


def _tiled(dual, bk, tm):
    return f"mfma_tiled<dual={dual},bk={bk},tm={tm}>"


ALL_INSTANTIATIONS = [_stream(d, s, x, t) for x in (1, 0) for t in (1, 2, 4) for s in (0, 1) for d in (0, 1)] + \
                     [_tiled(1, 64, 64), _tiled(1, 32, 64), _tiled(0, 128, 64), _tiled(0, 128, 128), _tiled(0, 32, 128), _tiled(1, 32, 128)]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """One vv_linear call.  pro: none | rms (weight) | rms_now (no weight) | silu; mod: None | "2k" | "3k" (shift, scale side by side in one
    [m, ld_mod] array, as the head's adaLN output) | "k+4" (two arrays); gate: None | "chan" (gate_ld 0) | "n+4" | "3n" (third block of a [m, 3n]
    array); res: None | "out" (its own array) | "inplace" (res == out); scalar: None (vector epilogue where n allows) | "ld" (ldo = ldres = n + 1)
    | "ptr" (out 4 bytes past a 16-byte boundary); ldx: row pitch of x when rows overlap (ldx < k), else k + 8."""

    def __init__(self, cid, route, m, n, k, xb=True, pro="none", mod=None, bias=False, act="none", gate=None, res=None, out_bf16=False,
                 scalar=None, ldx=None, hooks=None):
        self.id, self.route, self.m, self.n, self.k, self.xb, self.pro, self.mod, self.bias, self.act = cid, route, m, n, k, xb, pro, mod, bias, act
        self.gate, self.res, self.out_bf16, self.scalar, self.ldx, self.hooks = gate, res, out_bf16, scalar, ldx, dict(hooks or {})
        self.dual = act == "swiglu"
        assert not (xb and pro != "none") and not (mod and not pro.startswith("rms")) and not (res == "inplace" and out_bf16)

    @property
    def klass(self):
        if self.out_bf16:
            return "bf16"
        if self.xb:
            return "xb"
        return {"none": "none", "silu": "silu"}.get(self.pro, "rms_mod" if self.mod else "rms")

    @property
    def data_key(self):      # everything the VALUES depend on: layout (scalar, gap widths) and tune hooks are not part of it
        return (self.m, self.n, self.k, self.xb, self.pro, bool(self.mod), self.bias, self.act, "row" if self.gate in ("n+4", "3n") else self.gate,
                bool(self.res), self.out_bf16, self.ldx)


def _cases():
    cs = []

    def add(cid, route, m, n, k, **kw):
        cs.append(Case(cid, route, m, n, k, **kw))

    # ---- tiled kernels: xb, m = 161 (128 + 33: the last 64- and 128-row tile holds one row in its second wave row), n = 1536 (24 tiles) ----
    T = []      # (id, route, m, n, k, kw) - run again on the streaming kernels at hook mfma_tiled_rows 0
    T.append(("t_d64_k192", _tiled(1, 64, 64), 161, 1536, 192, dict(act="swiglu")))
    T.append(("t_d64_k576", _tiled(1, 64, 64), 161, 1536, 576, dict(act="swiglu")))
    T.append(("t_d64_k192_bf16out", _tiled(1, 64, 64), 161, 1536, 192, dict(act="swiglu", out_bf16=True)))
    T.append(("t_d32q_k96", _tiled(1, 32, 64), 161, 1536, 96, dict(act="swiglu")))
    T.append(("t_d32q_k352", _tiled(1, 32, 64), 161, 1536, 352, dict(act="swiglu")))
    T.append(("t_q_k1024_bias_res", _tiled(0, 128, 64), 161, 1536, 1024, dict(bias=True, res="out")))
    T.append(("t_q_k1152_bias_res_inplace", _tiled(0, 128, 64), 161, 1536, 1152, dict(bias=True, res="inplace")))
    T.append(("t_l_k128_bias", _tiled(0, 128, 128), 161, 1536, 128, dict(bias=True)))
    T.append(("t_l_k640", _tiled(0, 128, 128), 161, 1536, 640, dict()))
    T.append(("t_l_k640_gelu_bf16out", _tiled(0, 128, 128), 161, 1536, 640, dict(bias=True, act="gelu", out_bf16=True)))
    T.append(("t_l_k128_gate_res", _tiled(0, 128, 128), 161, 1536, 128, dict(gate="chan", res="out")))
    T.append(("t_s_k32", _tiled(0, 32, 128), 161, 1536, 32, dict()))
    T.append(("t_s_k96", _tiled(0, 32, 128), 161, 1536, 96, dict(bias=True)))
    T.append(("t_s_k288", _tiled(0, 32, 128), 161, 1536, 288, dict()))
    T.append(("t_s_k224_overlap", _tiled(0, 32, 128), 161, 1536, 224, dict(bias=True, ldx=64)))
    T.append(("t_narrow_64x64", _tiled(0, 128, 64), 64, 64, 8192, dict()))
    T.append(("t_narrow_70x192_bias", _tiled(0, 128, 64), 70, 192, 8192, dict(bias=True)))
    T.append(("t_fewrows_33", _tiled(0, 128, 128), 33, 3072, 128, dict(bias=True)))
    for cid, route, m, n, k, kw in T:
        add(cid, route, m, n, k, **kw)
    add("t_dbig_k96_hook", _tiled(1, 32, 128), 161, 1536, 96, act="swiglu", hooks={"mfma_tiled_small_dual": 0})
    add("t_dbig_256tiles", _tiled(1, 32, 128), 1024, 4096, 64, act="swiglu")
    add("t_bk128off_k640", _tiled(0, 32, 128), 161, 1536, 640, hooks={"mfma_tiled_bk128": 0})
    add("t_dualbk64off_k192", _tiled(1, 32, 64), 161, 1536, 192, act="swiglu", hooks={"mfma_tiled_dual_bk64": 0})
    add("t_smalloff_k1024", _tiled(0, 128, 128), 161, 1536, 1024, bias=True, res="out", hooks={"mfma_tiled_small": 0})
    # the same operands on the streaming kernels: the one place where tiled and streaming results of identical operands sit side by side
    for cid, _, m, n, k, kw in T:
        dual = int(kw.get("act") == "swiglu")
        mt = 4 if (m >= 128 and k >= 1024 and n >= 1024) else 1
        ks = int(k >= 512 or (((n + 31) // 32) * ((m + 32 * mt - 1) // (32 * mt)) < 256 and k >= 128))
        add("s_" + cid[2:] + "_rows0", _stream(dual, ks, 1, mt), m, n, k, hooks={"mfma_tiled_rows": 0}, **kw)

    # ---- streaming kernels, bf16 x ----
    add("x_ks0_6steps", _stream(0, 0, 1, 1), 70, 100, 96, bias=True, res="out")                 # 6 steps < unroll 8, last wave holds 4 channels
    add("x_ks0_k16_scalar", _stream(0, 0, 1, 1), 70, 70, 16, bias=True, gate="chan", res="out")  # ldo = 74: scalar epilogue
    add("x_ks0_n1", _stream(0, 0, 1, 1), 70, 1, 32, bias=True)
    add("x_ks0_9steps", _stream(0, 0, 1, 1), 129, 2052, 144)                                     # 9 steps = 8 + 1
    add("x_ks0_gelu_gate_ptr", _stream(0, 0, 1, 1), 70, 100, 96, bias=True, act="gelu", gate="n+4", res="out", scalar="ptr")
    add("x_ks1_9steps", _stream(0, 1, 1, 1), 70, 100, 144, bias=True, res="inplace")            # 9 steps over 4 waves: the last wave gets none
    add("x_ks1_k160", _stream(0, 1, 1, 1), 70, 100, 160, gate="chan")
    add("x_ks1_longk", _stream(0, 1, 1, 1), 70, 36, 8208, bias=True)                             # long K that the narrow entry declines
    add("x_ks1_gelu_bf16out", _stream(0, 1, 1, 1), 70, 100, 144, bias=True, act="gelu", out_bf16=True)
    add("x_ks1_gelu_bf16out_ld", _stream(0, 1, 1, 1), 70, 100, 144, bias=True, act="gelu", out_bf16=True, scalar="ld")
    add("x_ks1_overlap", _stream(0, 1, 1, 1), 70, 100, 224, bias=True, ldx=64)
    add("x_ks0_dual", _stream(1, 0, 1, 1), 70, 100, 96, act="swiglu")
    add("x_ks0_dual_ld", _stream(1, 0, 1, 1), 70, 100, 96, act="swiglu", scalar="ld")
    add("x_ks1_dual", _stream(1, 1, 1, 1), 70, 100, 144, act="swiglu")
    add("x_ks1_dual_bf16out", _stream(1, 1, 1, 1), 70, 100, 144, act="swiglu", out_bf16=True)
    add("x_mt4_plain", _stream(0, 1, 1, 4), 161, 1028, 1040, bias=True, res="out")              # strips of 128 + 33 rows, last block 4 channels, 65 steps 17/17/17/14
    add("x_mt4_dual", _stream(1, 1, 1, 4), 161, 1028, 1040, act="swiglu")
    add("x_mt4_ks0_hook", _stream(0, 0, 1, 4), 161, 4100, 144, hooks={"mfma_mt": 4})
    add("x_mt4_ks0_dual_hook", _stream(1, 0, 1, 4), 161, 100, 96, act="swiglu", hooks={"mfma_mt": 4})
    add("x_mt2_ks0_hook", _stream(0, 0, 1, 2), 161, 4100, 144, hooks={"mfma_mt": 2})
    add("x_mt2_ks0_dual_hook", _stream(1, 0, 1, 2), 161, 100, 96, act="swiglu", hooks={"mfma_mt": 2})
    add("x_mt2_ks1_hook", _stream(0, 1, 1, 2), 161, 100, 160, bias=True, res="out", hooks={"mfma_mt": 2})
    add("x_mt2_ks1_dual_hook", _stream(1, 1, 1, 2), 161, 100, 160, act="swiglu", hooks={"mfma_mt": 2})

    # ---- streaming kernels, fp32 x (staged activations): prologue x epilogue variants on a ksplit=0 and a ksplit=1 shape, vector and scalar ----
    V = [("none_bias_res", dict(bias=True, res="out")),
         ("rms_bias", dict(pro="rms", bias=True)),
         ("rmsnow_mod2k", dict(pro="rms_now", mod="2k")),
         ("rms_mod_rowgate_res", dict(pro="rms", mod="3k", gate="3n", res="inplace")),
         ("silu", dict(pro="silu")),
         ("rms_swiglu", dict(pro="rms", act="swiglu")),
         ("gelu_gate_res", dict(bias=True, act="gelu", gate="chan", res="out")),
         ("rms_gelu_bf16out", dict(pro="rms", bias=True, act="gelu", out_bf16=True))]
    for vi, (name, kw) in enumerate(V):
        dual = int(kw.get("act") == "swiglu")
        for ks, k in ((0, 96), (1, 144)):
            add(f"f_{name}_ks{ks}", _stream(dual, ks, 0, 1), 40, 100, k, xb=False, **kw)
            add(f"f_{name}_ks{ks}_scalar", _stream(dual, ks, 0, 1), 40, 100, k, xb=False, scalar=("ld", "ptr")[(vi + ks) % 2], **kw)
    add("f_rms_modk4_rowgate", _stream(0, 1, 0, 1), 40, 100, 144, xb=False, pro="rms", mod="k+4", gate="n+4")
    add("f_none_k1040", _stream(0, 1, 0, 1), 40, 100, 1040, xb=False, bias=True, res="out")     # LDS chunks 1024 + 16
    add("f_rms_k1040", _stream(0, 1, 0, 1), 40, 100, 1040, xb=False, pro="rms", bias=True)
    add("f_silu_k1040", _stream(0, 1, 0, 1), 40, 100, 1040, xb=False, pro="silu")
    add("f_rms_mod_k2064", _stream(0, 1, 0, 1), 40, 100, 2064, xb=False, pro="rms", mod="3k", gate="3n", res="out")   # 1024 + 1024 + 16
    add("f_mt2_rms_bias", _stream(0, 1, 0, 2), 161, 1028, 1040, xb=False, pro="rms", bias=True)  # the unhooked MT = 2 kernel: chunks 512 + 512 + 16
    add("f_mt2_rms_swiglu", _stream(1, 1, 0, 2), 161, 1028, 1040, xb=False, pro="rms", act="swiglu")
    add("f_mt2_ks0_hook", _stream(0, 0, 0, 2), 70, 100, 96, xb=False, pro="rms", bias=True, hooks={"mfma_mt": 2})
    add("f_mt2_ks0_dual_hook", _stream(1, 0, 0, 2), 70, 100, 96, xb=False, pro="rms", act="swiglu", hooks={"mfma_mt": 2})
    add("f_mt4_k528_hook", _stream(0, 1, 0, 4), 161, 100, 528, xb=False, pro="rms", bias=True, hooks={"mfma_mt": 4})   # chunks 256 + 256 + 16
    add("f_mt4_k528_dual_hook", _stream(1, 1, 0, 4), 161, 100, 528, xb=False, pro="rms", act="swiglu", hooks={"mfma_mt": 4})
    add("f_mt4_ks0_hook", _stream(0, 0, 0, 4), 161, 100, 96, xb=False, bias=True, res="out", hooks={"mfma_mt": 4})
    add("f_mt4_ks0_dual_hook", _stream(1, 0, 0, 4), 161, 100, 96, xb=False, pro="rms", act="swiglu", hooks={"mfma_mt": 4})
    add("f_overlap", _stream(0, 1, 0, 1), 40, 48, 224, xb=False, bias=True, res="out", ldx=64)
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
# three fixed shapes whose default routes a leaked vv_tune setting would change
HYGIENE = [("t_q_k1024_bias_res", _tiled(0, 128, 64)), ("t_d64_k192", _tiled(1, 64, 64)), ("x_mt4_plain", _stream(0, 1, 1, 4))]


def instantiation_table():
    lines = []
    for inst in ALL_INSTANTIATIONS:
        ids = [c.id for c in CASES if c.route == inst]
        text = ", ".join(ids[:4]) + (f", ... ({len(ids)} cases)" if len(ids) > 4 else "")
        lines.append(f"  {inst:<42} {text}")
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# operands, the fp64 reference and the fp32 stand-in (CPU)
# ---------------------------------------------------------------------------------------------------------------
def bf16_round64(t):
    """fp64 -> the nearest bf16 value (ties to even), returned as fp64: ONE rounding (torch's double -> bfloat16 goes through float).  Normal range only."""
    a = t.double().numpy()
    mant, e = np.frexp(a)                      # a = mant 2^e, |mant| in [0.5, 1): bf16 keeps 8 significant bits
    return torch.from_numpy(np.ldexp(np.round(mant * 256.0) / 256.0, e))


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    m, n, k, xb, pro, mod, bias, act, gate, res, out_bf16, ldx = key
    g = torch.Generator().manual_seed(zlib.crc32(repr((m, n, k, xb, pro, act, ldx or 0)).encode()))
    o = {}
    if ldx:                                     # overlapping rows: one flat buffer, row r starts at r * ldx
        flat = torch.randn((m - 1) * ldx + k, generator=g)
        flat = flat.bfloat16() if xb else flat
        o["x_flat"], o["x"] = flat, flat.as_strided((m, k), (ldx, 1))
    else:
        x = torch.randn(m, k, generator=g)
        o["x"] = x.bfloat16() if xb else x
    o["w"] = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    if act == "swiglu":
        o["w2"] = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
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


def _prologue(x, o, pro, dt, eps=EPS):
    """prologue of vv_linear in dtype dt, in the kernel's order of operations"""
    x = x.to(dt)
    if pro in ("rms", "rms_now"):
        x = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
        if "norm_w" in o:
            x = x * o["norm_w"].to(dt)
        if "scale" in o:
            x = x * (1 + o["scale"].to(dt)) + o["shift"].to(dt)
    elif pro == "silu":
        x = x / (1 + torch.exp(-x))
    return x


def _epilogue(y, y2, o, act, dt, rs=slice(None), cs=slice(None)):
    if "bias" in o:
        y = y + o["bias"][cs].to(dt)
    if act == "gelu":
        y = 0.5 * y * (1 + torch.erf(y * 0.70710678118654752440))
    elif act == "swiglu":
        y = y / (1 + torch.exp(-y)) * y2
    if "gate" in o:
        y = y * (o["gate"][cs] if o["gate"].dim() == 1 else o["gate"][rs, cs]).to(dt)
    if "res" in o:
        y = y + o["res"][rs, cs].to(dt)
    return y


def ref_linear_fp64(o, pro="none", act="none", out_bf16=False, xb=False, round_act=True):
    """vv_linear in plain fp64 on the operands as the device receives them.  round_act=False leaves the activations unrounded (only to compare
    this function with _ref_linear of test_hip_parity.py, which never rounds)."""
    x = o["x"].double() if xb else _prologue(o["x"], o, pro, torch.float64)
    if not xb and round_act:
        x = bf16_round64(x)
    y = x @ o["w"].double().t()
    y2 = x @ o["w2"].double().t() if "w2" in o else None
    y = _epilogue(y, y2, o, act, torch.float64)
    return bf16_round64(y) if out_bf16 else y


def _steps16(xh, w):
    """fp32 partial products of the 16-wide K steps: P[s] = xh[:, 16 s : 16 s + 16] @ w[:, same].T"""
    (m, k), n = xh.shape, w.shape[0]
    return torch.bmm(xh.reshape(m, k // 16, 16).transpose(0, 1), w.float().reshape(n, k // 16, 16).permute(1, 2, 0))


def _accumulate(P, skip=None, rs=slice(None), cs=slice(None)):
    acc = torch.zeros_like(P[0][rs, cs])
    for s in range(P.shape[0]):
        if s != skip:
            acc = acc + P[s][rs, cs]
    return acc


def tile_row_errors(got, ref, tm=32, tn=32):
    """(worst rel RMS over aligned tm x tn tiles (32 x 32 unless given) cut at the edges, its tile index, worst rel RMS over rows, its row) of
    got against ref (fp64)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e2, r2 = (got - ref) ** 2, ref ** 2
    m, n = ref.shape
    mp, npad = -(-m // tm) * tm, -(-n // tn) * tn

    def tiles(a):
        p = np.zeros((mp, npad))
        p[:m, :n] = a
        return p.reshape(mp // tm, tm, npad // tn, tn).sum((1, 3))

    t = np.sqrt(tiles(e2) / (tiles(r2) + 1e-300))
    r = np.sqrt(e2.sum(1) / (r2.sum(1) + 1e-300))
    ti = np.unravel_index(np.argmax(t), t.shape)
    return float(t.max()), (int(ti[0]), int(ti[1])), float(r.max()), int(np.argmax(r))


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / (np.sqrt(np.mean(b ** 2)) + 1e-300))


@functools.lru_cache(maxsize=None)
def _expect_of(key):
    """(fp64 reference, floor (global, tile, row) of the fp32 stand-in, cost of one dropped 16-wide K step in one tile) for one set of operands"""
    m, n, k, xb, pro, mod, bias, act, gate, res, out_bf16, ldx = key
    o = _operands_of(key)
    ref = ref_linear_fp64(o, pro, act, out_bf16, xb)
    xh = o["x"].float() if xb else _prologue(o["x"], o, pro, torch.float32).bfloat16().float()
    P = _steps16(xh, o["w"])
    P2 = _steps16(xh, o["w2"]) if "w2" in o else None

    def finish(y, y2, rs=slice(None), cs=slice(None)):
        y = _epilogue(y, y2, o, act, torch.float32, rs, cs)
        return (y.bfloat16() if out_bf16 else y).double()

    stand = finish(_accumulate(P), _accumulate(P2) if P2 is not None else None)
    t, _, r, _ = tile_row_errors(stand, ref)
    floor = (_rel(stand, ref), t, r)
    S, drop = k // 16, math.inf
    rs, cs = slice(0, min(32, m)), slice(0, min(32, n))                          # the first tile; the cheapest of the first, middle and last step
    for s0 in {0, S // 2, S - 1}:
        y = finish(_accumulate(P, s0, rs, cs), _accumulate(P2, s0, rs, cs) if P2 is not None else None, rs, cs)
        drop = min(drop, _rel(y, ref[rs, cs]))
    return ref, floor, drop


def expect(case):
    return _expect_of(case.data_key)


# ---------------------------------------------------------------------------------------------------------------
# CPU-only guards
# ---------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_ref_linear_of_the_parity_suite():
    """Guards the reference (CPU only): against _ref_linear of test_hip_parity.py it is exact on bf16 activations (nothing to round), and with
    the one bf16 rounding of the activations switched off it is the same function for an RMSNorm + modulate + GELU + gate + residual call."""
    from test_hip_parity import _ref_linear
    a = Case("g1", "", 24, 40, 64, xb=True, bias=True, act="gelu", gate="chan", res="out")
    o = operands(a)
    want = _ref_linear(o["x"].float(), o["w"].float(), None, o["bias"], 0, None, EPS, None, None, 1, o["gate"], o["res"])
    e = rel_rms(ref_linear_fp64(o, "none", "gelu", False, True).numpy(), want.numpy(), "fp64 reference vs _ref_linear, bf16 x (CPU)")
    assert e < 1e-12, e
    b = Case("g2", "", 24, 40, 64, xb=False, pro="rms", mod="2k", bias=True, act="gelu", gate="n+4", res="out")
    o = operands(b)
    want = _ref_linear(o["x"], o["w"].float(), None, o["bias"], 1, o["norm_w"], EPS, o["shift"], o["scale"], 1, o["gate"], o["res"])
    e = rel_rms(ref_linear_fp64(o, "rms", "gelu", False, False, round_act=False).numpy(), want.numpy(), "fp64 reference (unrounded) vs _ref_linear (CPU)")
    assert e < 1e-12, e
    c = Case("g3", "", 24, 40, 64, xb=False, pro="rms", act="swiglu")
    o = operands(c)
    want = _ref_linear(o["x"], o["w"].float(), o["w2"].float(), None, 1, o["norm_w"], EPS, None, None, 2, None, None)
    e = rel_rms(ref_linear_fp64(o, "rms", "swiglu", False, False, round_act=False).numpy(), want.numpy(), "fp64 reference (unrounded, SwiGLU) vs _ref_linear (CPU)")
    assert e < 1e-12, e
    # and the rounding it adds is one bf16 rounding of the activations, no more: ~ 2^-9 / sqrt(3) of the result
    e = _rel(ref_linear_fp64(o, "rms", "swiglu").numpy(), want.numpy())
    assert 2e-4 < e < 4e-3, e


def test_bf16_round64_is_one_round_to_nearest_even():
    v = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -40, 1.998046875, -0.0, 2.0 ** -126, 3.140625, -1 - 2.0 ** -8 - 2.0 ** -30], dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 2.0, -0.0, 2.0 ** -126, 3.140625, -1 - 2.0 ** -7], dtype=torch.float64)
    assert torch.equal(bf16_round64(v), want)
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    assert torch.equal(bf16_round64(x), x.bfloat16().double())      # from fp32 there is no double rounding: torch agrees


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_step(cid):
    """Both conditions on the class bar, for every case of the file (CPU only): at least 8 x the fp32 stand-in's own error against the fp64
    reference (global, worst tile, worst row), at most a tenth of what one dropped 16-wide K step costs the tile it is dropped from."""
    case = CASES[CASE_IDS.index(cid)]
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} tile {floor[1]:.2e} row {floor[2]:.2e}  dropped step {drop:.2e}")
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


def test_docstring_table_is_current():
    """the instantiation -> case table of the docstring is the one the parametrisation generates, and names all 30 instantiations"""
    assert instantiation_table() in __doc__
    routes = {c.route for c in CASES}
    assert routes == set(ALL_INSTANTIATIONS) and len(ALL_INSTANTIATIONS) == 30, routes ^ set(ALL_INSTANTIATIONS)


def built_kernels(unit, tmp_path, plain=False):
    """(kernel template, [template arguments]) of every kernel descriptor (*.kd) in the gfx950 code object of one translation unit's object file
    under build.OBJDIR - what the device compiler generated, whatever the host side still launches.  Symbol names only: the .hip_fatbin section is
    copied out, the gfx950 bundle unpacked and its symbol table listed, with the LLVM tools that sit next to hipcc.  plain: kernels that are no
    templates are listed too, as (name, [])."""
    from vibevoice_rocm_amd import build as vb
    obj = vb._obj(os.path.join(vb.HERE, "csrc", unit))
    assert os.path.exists(obj), f"{obj} is missing: build() leaves one object file per translation unit there"
    hip = os.path.dirname(os.path.realpath(vb.find_hipcc()))
    dirs = [os.environ.get("HIP_CLANG_PATH"), os.path.join(hip, "..", "lib", "llvm", "bin"), os.path.join(hip, "..", "llvm", "bin"), hip]

    def tool(name):
        found = next((os.path.join(d, name) for d in dirs if d and os.path.exists(os.path.join(d, name))), None) or shutil.which(name)
        assert found, f"{name} not found next to hipcc"
        return found

    fatbin, co = str(tmp_path / (unit + ".fatbin")), str(tmp_path / (unit + ".co"))
    subprocess.run([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fatbin], check=True)
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fatbin,
                    "--output=" + co], check=True)
    syms = subprocess.run([tool("llvm-readelf"), "--symbols", "--wide", "--demangle", co], check=True, capture_output=True, text=True).stdout
    out = []
    for line in syms[syms.index("Symbol table '.symtab'"):].splitlines():      # the listing holds .dynsym too: every kernel would come twice
        hit = re.search(r"(\w+)<(.*)>\(.*\) \(\.kd\)$", line)
        if hit:
            out.append((hit.group(1), hit.group(2).split(", ")))
        elif plain:
            hit = re.search(r"(\w+)\([^<>]*\) \(\.kd\)$", line)
            if hit:
                out.append((hit.group(1), []))
    return out


def instantiations_of(kernels, names):
    """The route names of the built kernels whose template is a key of `names` (template -> function of its arguments as ints; bools 0 / 1, the
    weight types by name); every name once, or the build holds a kernel twice"""
    val = {"true": 1, "false": 0, "float": "f32", "unsigned short": "bf16"}
    got = [names[k](*[val[a] if a in val else int(a) for a in args]) for k, args in kernels if k in names]
    assert len(set(got)) == len(got)
    return set(got)


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """vv_mfma_gemm.hip's code object holds the 30 kernels of ALL_INSTANTIATIONS and no other instantiation of the two templates (CPU only: reads
    the symbol table of the object file build() left)"""
    got = instantiations_of(built_kernels("vv_mfma_gemm.hip", tmp_path), {"mfma_linear_kernel": _stream, "mfma_tiled_kernel": _tiled})
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))


# ---------------------------------------------------------------------------------------------------------------
# the call: layout with NaN gaps and guards, route assertion, launch
# ---------------------------------------------------------------------------------------------------------------
NAN = float("nan")
_LIB = []


def _lib():
    if not _LIB:
        from vibevoice_rocm_amd import _lib as L
        _LIB.extend((L, L.load()))
    return _LIB


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    L, l = _lib()[:2]
    if len(_LIB) == 2:
        L.check(l.vv_init(), "vv_init")
        _LIB.append(True)


class _tuned:
    def __init__(self, hooks):
        self.hooks = hooks

    def __enter__(self):
        L, l = _lib()[:2]
        for key, v in self.hooks.items():
            assert key in TUNE_DEFAULTS
            L.check(l.vv_tune(key.encode(), v), "vv_tune")

    def __exit__(self, *exc):
        L, l = _lib()[:2]
        for key in self.hooks:
            L.check(l.vv_tune(key.encode(), TUNE_DEFAULTS[key]), "vv_tune")


def _gapped(t, ld, col0=0):
    """[rows, ld] filled with NaN, t in columns col0 .. col0 + t.shape[1]"""
    out = torch.full((t.shape[0], ld), NAN, dtype=t.dtype)
    out[:, col0: col0 + t.shape[1]] = t
    return out


def layout(case, o):
    """The host image of every array the call reads, NaN in every gap, and the strides: {name: tensor}, {field: stride}.  "out" is the
    initial image of the output allocation: (m + 2) rows of pitch ldo (two guard rows), all NaN - or the residual where res == out."""
    m, n, k = case.m, case.n, case.k
    buf, ld = {}, {}
    if case.ldx:
        buf["x"], ld["ldx"] = o["x_flat"], case.ldx
    else:
        buf["x"], ld["ldx"] = _gapped(o["x"], k + 8), k + 8
    buf["w"] = o["w"].contiguous()
    if "w2" in o:
        buf["w2"] = o["w2"].contiguous()
    for name in ("norm_w", "bias"):
        if name in o:
            buf[name] = o[name]
    if case.mod in ("2k", "3k"):
        ld["ld_mod"] = (2 if case.mod == "2k" else 3) * k
        mod = torch.full((m, ld["ld_mod"]), NAN)
        mod[:, :k], mod[:, k: 2 * k] = o["shift"], o["scale"]
        buf["mod"] = mod
    elif case.mod == "k+4":
        ld["ld_mod"] = k + 4
        buf["shift"], buf["scale"] = _gapped(o["shift"], k + 4), _gapped(o["scale"], k + 4)
    ld["gate_ld"] = {None: 0, "chan": 0, "n+4": n + 4, "3n": 3 * n}[case.gate]
    if case.gate == "chan":
        buf["gate"] = o["gate"]
    elif case.gate == "n+4":
        buf["gate"] = _gapped(o["gate"], n + 4)
    elif case.gate == "3n":
        buf["gate"] = _gapped(o["gate"], 3 * n, 2 * n)
    ldo = n + 1 if case.scalar == "ld" else n + 4
    ld["ldo"] = ld["ldres"] = ldo
    ld["out_off"] = 0 if case.scalar != "ptr" else (2 if case.out_bf16 else 1)       # elements: 4 bytes past the allocation's 16-byte boundary
    out = torch.full((ld["out_off"] + (m + 2) * ldo,), NAN, dtype=torch.bfloat16 if case.out_bf16 else torch.float32)
    if case.res == "inplace":
        out[ld["out_off"]:].view(m + 2, ldo)[:m, :n] = o["res"]
    elif case.res:
        buf["res"] = _gapped(o["res"], ldo)
    buf["out"] = out
    return buf, ld


def fill_args(case, ld, ptr):
    """vv_lin_args of the case; ptr: {name: address of the array layout() describes}"""
    L, _ = _lib()[:2]
    m, n, k = case.m, case.n, case.k
    esz = 2 if case.out_bf16 else 4
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.eps = ptr["x"], ld["ldx"], m, n, k, L.VV_BF16, ptr["w"], EPS
    a.flags = (L.LIN_X_BF16 if case.xb else 0) | (L.LIN_OUT_BF16 if case.out_bf16 else 0)
    a.pro = {"none": L.PRO_NONE, "rms": L.PRO_RMSNORM, "rms_now": L.PRO_RMSNORM, "silu": L.PRO_SILU}[case.pro]
    a.act = {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "swiglu": L.ACT_SWIGLU}[case.act]
    if case.pro == "rms":
        a.norm_w = ptr["norm_w"]
    if case.mod in ("2k", "3k"):
        a.mod_shift, a.mod_scale, a.ld_mod = ptr["mod"], ptr["mod"] + 4 * k, ld["ld_mod"]
    elif case.mod:
        a.mod_shift, a.mod_scale, a.ld_mod = ptr["shift"], ptr["scale"], ld["ld_mod"]
    if case.dual:
        a.w2 = ptr["w2"]
    if case.bias:
        a.bias = ptr["bias"]
    if case.gate:
        a.gate, a.gate_ld = ptr["gate"] + (4 * 2 * n if case.gate == "3n" else 0), ld["gate_ld"]
    a.out, a.ldo = ptr["out"] + esz * ld["out_off"], ld["ldo"]
    if case.res == "inplace":
        a.res, a.ldres = a.out, ld["ldo"]
    elif case.res:
        a.res, a.ldres = ptr["res"], ld["ldres"]
    return a


def route_of(a):
    L, l = _lib()[:2]
    name = C.create_string_buffer(96)
    L.check(l.vv_linear_route(C.byref(a), name, 96), "vv_linear_route")
    return name.value.decode()


_FAKE = {name: 0x10000000 * (i + 1) for i, name in enumerate(("x", "w", "w2", "norm_w", "bias", "mod", "shift", "scale", "gate", "res", "out"))}


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_case_on_the_host(cid):
    """The route query needs no device: every case's arguments (16-byte aligned stand-in addresses, nothing is dereferenced) report the
    instantiation the case is named for, here on the CPU too, and the tune state is back at its defaults afterwards."""
    case = CASES[CASE_IDS.index(cid)]
    _, ld = layout(case, operands(case))
    with _tuned(case.hooks):
        got = route_of(fill_args(case, ld, _FAKE))
    assert got == case.route, (cid, got, case.route)
    for hid, want in HYGIENE:
        h = CASES[CASE_IDS.index(hid)]
        assert route_of(fill_args(h, layout(h, operands(h))[1], _FAKE)) == want


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


_MEASURED = {}      # class -> [global, tile, row] maxima of this session, written by _report


def run_case(case):
    """Lay the case out, assert its route, launch it twice into separate outputs; returns (out[m, n] as fp64, got route)"""
    L, l = _lib()[:2]
    o = operands(case)
    buf, ld = layout(case, o)
    m, n, ldo, off = case.m, case.n, ld["ldo"], ld["out_off"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda(), buf["out"].cuda()]
    with _tuned(case.hooks):
        for i, out in enumerate(outs):
            a = fill_args(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
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


pytest_gpu = pytest.mark.gpu


@pytest_gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_mfma_gemm_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref, floor, drop = expect(case)
    got = run_case(case).numpy()
    g = rel_rms(got, ref.numpy(), f"{cid} [{case.route}] global")
    t, ti, r, ri = tile_row_errors(got, ref.numpy())
    bar = BAR[case.klass]
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst tile {t:.3e} at (row tile {ti[0]}, channel tile {ti[1]})  "
          f"worst row {r:.3e} (row {ri})  [floor {max(floor):.2e}, dropped step {drop:.2e}]")
    mx = _MEASURED.setdefault(case.klass, [0.0, 0.0, 0.0])
    for i, v in enumerate((g, t, r)):
        mx[i] = max(mx[i], v)
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert t < bar, f"{cid}: 32 x 32 tile (row tile {ti[0]}, channel tile {ti[1]}) rel RMS {t:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"


@pytest_gpu
def test_refusals_launch_nothing():
    """bf16 x with a prologue, with k % 16 != 0, and with ldx % 8 != 0 (the "not covered" error, no silent fp32 fallback reading bf16 as fp32):
    vv_linear_route and vv_linear both refuse, and the output is untouched."""
    _need_gpu()
    L, l = _lib()[:2]
    m, n, k = 40, 64, 64
    x = torch.randn(m, k + 8).bfloat16().cuda()
    w = torch.randn(n, k).bfloat16().cuda()
    nw = torch.ones(k).cuda()
    out = torch.full((m, n), NAN, device="cuda")
    name = C.create_string_buffer(96)

    def args(**kw):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo, a.flags, a.eps = x.data_ptr(), k + 8, m, n, k, L.VV_BF16, w.data_ptr(), out.data_ptr(), n, L.LIN_X_BF16, EPS
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    assert route_of(args()).startswith("mfma_")                     # the unspoiled call is covered
    for a, code, text in ((args(pro=L.PRO_RMSNORM, norm_w=nw.data_ptr()), -1, "no prologue"), (args(k=56), -1, "k % 16"), (args(ldx=k + 4), -3, "not covered")):
        for rc in (l.vv_linear_route(C.byref(a), name, 96), l.vv_linear(C.byref(a), None)):
            assert rc == code and text in l.vv_last_error().decode(), (rc, l.vv_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


def test_route_names_other_families():
    """CPU only (the query touches no device): the families outside vv_mfma_gemm.hip by name"""
    L, l = _lib()[:2]

    def route(m, n, k, wdt=L.VV_BF16, res=False):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo = _FAKE["x"], k, m, n, k, wdt, _FAKE["w"], _FAKE["out"], n
        if res:
            a.res, a.ldres = _FAKE["res"], n
        return route_of(a)

    assert route(40, 512, 2560) == "skinny<nst=20,nb=1>"
    assert route(40, 512, 2560, res=True) == _stream(0, 1, 0, 1)
    assert route(40, 512, 2560, wdt=L.VV_F32) == "gemm_f32<w=f32,dual=0,vec=1,tile=32>"
    assert route(33, 70, 56) == "gemm_f32<w=bf16,dual=0,vec=1,tile=32>"                  # k % 16 != 0: the matrix-core path declines
    # m <= 8: the GEMV kernel itself (tests/test_hip_gemv.py pins the whole family); 5 units at 8 rows split K over 4 waves
    assert route(8, 512, 2560, res=True) == "gemv_stream<m=8,dual=0,ksplit=4,ku=2,rw=2,wq=bf16>"
    assert route(1, 512, 96) == "gemv_stream<m=1,dual=0,ksplit=1,ku=1,rw=2,wq=bf16>"


@pytest_gpu
def test_zz_tune_state_is_back_at_its_defaults():
    """Hook hygiene: three fixed shapes report their default routes, so a vv_tune setting leaked by any test above fails here."""
    _need_gpu()
    for hid, want in HYGIENE:
        h = CASES[CASE_IDS.index(hid)]
        assert not h.hooks
        assert route_of(fill_args(h, layout(h, operands(h))[1], _FAKE)) == want, hid
    _report()


def _report():
    """the session's largest figures per route class, for the docstring and profiles/mfma_gemm_parity.txt (written only where VV_MFMA_PARITY_OUT says)"""
    path = os.environ.get("VV_MFMA_PARITY_OUT")
    if not path or not _MEASURED:
        return
    with open(path, "w") as f:
        f.write(f"{torch.cuda.get_device_name(0)}: largest rel RMS against fp64 over each route class's cases (tests/test_hip_mfma_gemm.py)\n")
        f.write(f"{'class':<9} {'cases':>5} {'bar':>8} {'global':>10} {'tile':>10} {'row':>10} {'bar / largest':>14}\n")
        for k in BAR:
            if k in _MEASURED:
                g, t, r = _MEASURED[k]
                f.write(f"{k:<9} {sum(c.klass == k for c in CASES):>5} {BAR[k]:>8.1e} {g:>10.2e} {t:>10.2e} {r:>10.2e} {BAR[k] / max(g, t, r):>14.1f}\n")


# ---------------------------------------------------------------------------------------------------------------
# vv_cast_rows_bf16: the producer of every bf16 x operand
# ---------------------------------------------------------------------------------------------------------------
CAST_SPECIALS = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 0.0, -0.0, 2.0 ** -126, -2.0 ** -126, 1.998046875, -255.5, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -7 - 2.0 ** -23]
CAST_CASES = [(rows, n, pro) for rows in (1, 70) for n in (16, 1000, 1536, 3584) for pro in ("none", "rms", "rms_now")]


@functools.lru_cache(maxsize=None)
def _cast_inputs(rows, n, pro):
    g = torch.Generator().manual_seed(rows * 10007 + n)
    x = torch.randn(rows, n, generator=g)
    if pro == "none":
        x[0, : len(CAST_SPECIALS)] = torch.tensor(CAST_SPECIALS)          # ties both ways, signed zeros, the smallest normal, a round-up into the next binade
    w = 1 + 0.1 * torch.randn(n, generator=g) if pro == "rms" else None
    x64 = x.double()
    if pro != "none":
        x64 = x64 * torch.rsqrt((x64 * x64).mean(-1, keepdim=True) + EPS)
        if w is not None:
            x64 = x64 * w.double()
    return x, w, bf16_round64(x64).to(torch.bfloat16)       # exact: the values are bf16 already


def _ulp_diff(a, b):
    """|difference| in bf16 ulps between two bf16 tensors of equal sign (sign-magnitude bit patterns)"""
    ia, ib = a.view(torch.int16).int(), b.view(torch.int16).int()
    return (ia - ib).abs()


@pytest.mark.parametrize("rows,n,pro", [c for c in CAST_CASES if c[2] != "none"])
def test_cast_stand_in_stays_under_the_flip_cap(rows, n, pro):
    """CPU only: the fp32 formulation of the RMSNorm cast differs from the fp64 reference by at most one bf16 ulp, on fewer than CAST_FLIP_CAP
    of the elements - so the cap leaves the device room for its own fp32 summation order and rsqrtf."""
    x, w, ref = _cast_inputs(rows, n, pro)
    v = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS)
    if w is not None:
        v = v * w
    d = _ulp_diff(v.bfloat16(), ref)
    assert int(d.max()) <= 1
    share = float((d != 0).float().mean())
    print(f"cast stand-in rows {rows} n {n} {pro}: {share:.2e} of the elements differ by one ulp")
    assert share * 4 <= CAST_FLIP_CAP or int((d != 0).sum()) <= 1, share       # a single flip among 16 elements is no share


@pytest_gpu
@pytest.mark.parametrize("rows,n,pro", CAST_CASES)
def test_cast_rows_bf16_vs_fp64(rows, n, pro):
    _need_gpu()
    L, l = _lib()[:2]
    x, w, ref = _cast_inputs(rows, n, pro)
    ldx, ldo = n + 4, n + 8
    xh = _gapped(x, ldx)
    xd, wd = xh.cuda(), (w.cuda() if w is not None else None)
    out = torch.full((rows + 2, ldo), NAN, dtype=torch.bfloat16, device="cuda")
    L.check(l.vv_cast_rows_bf16(xd.data_ptr(), ldx, rows, n, L.PRO_NONE if pro == "none" else L.PRO_RMSNORM, L.ptr(wd), EPS, out.data_ptr(), ldo, None),
            "vv_cast_rows_bf16")
    torch.cuda.synchronize()
    h = out.cpu()
    assert _same_bits(xd.cpu(), xh) and (w is None or _same_bits(wd.cpu(), w))
    assert torch.isnan(h[:rows, n:]).all() and torch.isnan(h[rows:]).all(), "a gap or guard element was written"
    got = h[:rows, :n]
    if pro == "none":
        assert _same_bits(got.contiguous(), ref), "PRO_NONE is not bit-exact round-to-nearest-even"
        return
    assert torch.isfinite(got.float()).all()
    d = _ulp_diff(got.contiguous(), ref)
    share = float((d != 0).float().mean())
    print(f"cast rows {rows} n {n} {pro}: worst {int(d.max())} ulp, {share:.2e} of the elements differ")
    assert int(d.max()) <= 1, f"an element is {int(d.max())} bf16 ulps from the fp64 reference"
    assert share <= CAST_FLIP_CAP or int((d != 0).sum()) <= 1, share


if __name__ == "__main__":
    if "--table" in sys.argv:
        print(instantiation_table())

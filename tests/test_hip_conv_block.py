"""The conv tokenizers' Block1D kernels (vv_block_mixer, vv_block1d, vv_block_mid and the one-row stage) against one fp64 reference, per tile and
per row - through the C ABI only, no engine, no checkpoint.  Method and helpers are those of tests/test_hip_mfma_gemm.py.

Each call first asks the route query of its entry point (vv_block_mixer_route, vv_block1d_route, vv_block_mid_route) which kernel its arguments
take and asserts the kernel the case is named for.  The reference (`ref_block_fp64`) is plain torch fp64 of Block1D.forward on the operands as
the device receives them and knows nothing of tiles: RMSNorm, the causal 7-tap depthwise conv over [history ; rows] and the layer scale in fp64,
the FFN input rounded to bf16 once, GELU in the erf form, the hidden activation rounded to bf16 once, the second GEMM and the epilogue in fp64.

Every case is a sequence of calls on ONE history buffer: streaming with T, two different short streaming calls (after which the history is part
old rows, part new rows), streaming with T again, and one stateless call of T rows (zero left context, nothing stored).  vv_block1d refuses
T < 32, so its short calls are vv_block_mixer calls on the same history, as the composites make them.  Per call and quantity three figures:
global rel RMS, the worst aligned tile (edge tiles cut at T) and the worst row, for
  y        the mixer output, where the call exposes it (vv_block_mixer's out, the start of vv_block_mid's ws): fp32 arithmetic only; 16 x 16 tiles
  hid      the bf16 hidden activation behind it in vv_block_mid's ws, against the bf16-rounded reference; 16 rows x 32 hidden channels
  branch   out - y_ref against out_ref - y_ref: the FFN branch (and, for vv_block1d, whatever its mixer got wrong) without the residual that
           divides its error in `out`; 16 x 16 tiles
  out      the whole output, the weaker figure the older tests hold
  hist     the new history after every streaming call, worst row
Bars: per (family, quantity) class, and channel count where the arithmetic depends on it, one constant for the global and the worst-tile figure
and one for the worst-row figure (BAR): each fault below belongs to one of the two figures, and a flipped bf16 rounding of one FFN input moves a
whole row of the branch, so the row figure's floor lies above a tenth of what the GEMM faults cost their tile.
`test_bars_sit_between_floor_and_faults` (CPU) holds every case to both conditions of the mfma file - bar >= 8 x the error of a torch fp32
stand-in (fp32 prologue, rounded where the kernel rounds, accumulated in 16-wide K steps) against the reference, bar <= 1/10 of what each of these
faults, put into the stand-in, costs the figure meant to catch it:
  (a) one 16-wide K step of the second GEMM dropped in one 16 x 16 tile                      branch, worst tile
  (b) one K step of the first GEMM dropped in one 32-channel hidden block of one row tile    hid (vv_block_mid) / branch (vv_block1d), worst tile
  (c) one halo row of a row tile other than the first replaced by the row before it          y (branch for vv_block1d), worst row
  (d) the stored history shifted by one row                                                  hist, and y (branch) of the next call, worst row
  (e) two adjacent taps swapped in one group of 4 channels                                   y (branch for vv_block1d), worst tile
No (kernel, fault) pair had to be dropped.

Every GPU case keeps NaN guard rows in front of and behind each output and the history, 0xFF guard bytes around the workspace, runs every call
twice on two separate sets of buffers (bit-identical), and checks after each call that every guard is untouched, every in-range output is
finite and every input - x, the ten parameter arrays and, for a stateless call, the history - is bit-unchanged.  Each call waits for the device
under its own time limit (CALL_LIMIT_S).  The one-row stage (C = 2048) runs RowNet of tests/test_hip_conv_hot.py for 8 frames in the three modes
of test_one_row_stage_state_paths_1p5b_vs_oracle; its state tensors belong to the net and carry no guards.

Hooks: the file sets vv_tune hooks only through `_tuned`, which keeps a ledger; the last test asserts the ledger is at the defaults and that
five fixed shapes report their default routes (convffn_t1 / convffn_t1hs have no route query: for them the ledger is the check).

vv_block_mixer at C = 2048 with 16..256 stateless rows takes mixer_rows<tr=2,colfix=0>: two rows per workgroup is the smallest tile the
launcher's loop reaches at T >= 16, a one-row form does not exist.

Measured on the MI355X, largest value over the class's calls, global / worst tile / worst row rel RMS against fp64 (profiles/conv_block_parity.txt):
  class                  calls  bar tile   bar row     global       tile        row  bar / largest
  mixer y                   70   1.0e-05   1.0e-05   4.44e-08   8.87e-08   6.28e-08          112.7
  mixer hist                56   1.0e-05   1.0e-05   7.41e-08   1.15e-07   1.15e-07           87.1
  block1d branch            51   7.0e-03   3.0e-02   3.53e-04   6.48e-04   2.97e-03           10.1
  block1d out               51   7.0e-03   3.0e-02   1.07e-04   2.19e-04   6.69e-04           31.9
  block1d hist              68   1.0e-05   1.0e-05   7.12e-08   1.14e-07   1.14e-07           87.8
  mid y                    175   1.0e-05   1.0e-05   4.12e-08   1.03e-07   7.13e-08           97.0
  mid hist                 156   1.0e-05   1.0e-05   7.39e-08   1.15e-07   1.15e-07           86.8
  mid hid 128               45   1.5e-02   2.5e-02   2.73e-04   1.29e-03   2.49e-03           10.1
  mid hid 256               60   1.2e-02   1.2e-02   9.47e-05   1.09e-03   1.24e-03            9.7
  mid hid 512               60   1.2e-02   1.2e-02   1.65e-04   1.36e-03   1.67e-03            7.2
  mid hid 1024              30   8.0e-03   1.2e-02   5.44e-05   6.06e-04   2.29e-04           13.2
  mid branch 128            45   9.0e-03   2.5e-02   2.80e-04   1.08e-03   3.20e-03            7.8
  mid branch 256            60   7.0e-03   1.5e-02   1.00e-04   5.07e-04   1.44e-03           10.4
  mid branch 512            60   4.5e-03   1.0e-02   1.83e-04   6.84e-04   1.82e-03            5.5
  mid branch 1024           30   4.0e-03   1.0e-02   5.15e-05   1.65e-04   2.22e-04           24.3
  mid out 128               45   9.0e-03   2.5e-02   8.72e-05   2.92e-04   8.33e-04           30.0
  mid out 256               60   7.0e-03   1.5e-02   3.08e-05   1.44e-04   4.34e-04           34.5
  mid out 512               60   4.5e-03   1.0e-02   5.51e-05   2.17e-04   5.49e-04           18.2
  mid out 1024              30   4.0e-03   1.0e-02   1.57e-05   5.04e-05   7.27e-05           79.4
  row1 out                  24   2.0e-03   2.0e-03   9.17e-07   0.00e+00   9.17e-07         2181.0
  row1 state                24   2.0e-03   2.0e-03   1.69e-07   0.00e+00   1.67e-07        11830.6
Within a factor of ten of a bar: the hid and branch figures of vv_block_mid (hid 9.7 / 7.2 x below at C = 256 / 512, branch 7.8 / 5.5 x at
C = 128 / 512).  Each is a row (or the edge tile of a few rows that holds it) whose FFN input the device's fp32 prologue rounds to the other bf16
neighbour than the fp64 reference does: that moves every pre-activation of the row, a share of the row's 4C hidden values flips by one bf16 step,
and the branch inherits
it through W2 (the arithmetic is at BAR).  The CPU stand-in, which knows nothing of the device, shows rows of the same size (2.5e-3 for hid at
C = 128, 2.2e-3 for the branch); the y figure of the same calls, which has no rounding in it, is 1e-7.

Kernel -> case ids (generated: `python tests/test_hip_conv_block.py --table`; `test_docstring_table_is_current` keeps it so):
  block_mixer_kernel                       mx_s_1x2048, mx_s_5x96, mx_s_3x30, mx_s_33x48, ... (27 cases)
  mixer_rows_kernel                        mx_r_16x256, mx_r_17x1024, mx_r_40x512, mx_r_256x256, ... (7 cases)
  block1d<c=32>                            b1_c32_t32, b1_c32_t33, b1_c32_t37, b1_c32_t45, ... (5 cases)
  block1d<c=64>                            b1_c64_t32, b1_c64_t33, b1_c64_t37, b1_c64_t45, ... (5 cases)
  block1d<c=128>                           b1_c128_t32, b1_c128_t33, b1_c128_t37, b1_c128_t45, ... (7 cases)
  ffn_in<c=128,trv=16,nt=256>              mid_c128_trv16_t3, mid_c128_trv16_t17, mid_c128_trv16_t37
  ffn_in<c=128,trv=32,nt=256>              mid_c128_trv32_t3, mid_c128_trv32_t33, mid_c128_trv32_t69, mid_c128_trv32_t800, ... (6 cases)
  ffn_in<c=256,trv=8,nt=256>               mid_c256_trv8_t3, mid_c256_trv8_t9, mid_c256_trv8_t21
  ffn_in<c=256,trv=16,nt=256>              mid_c256_trv16_t3, mid_c256_trv16_t17, mid_c256_trv16_t37, mid_c256_trv16_t200, ... (6 cases)
  ffn_in<c=256,trv=32,nt=256>              mid_c256_trv32_t3, mid_c256_trv32_t33, mid_c256_trv32_t69
  ffn_in<c=512,trv=8,nt=512>               mid_c512_trv8_t3, mid_c512_trv8_t9, mid_c512_trv8_t21, mid_c512_trv8_t40, ... (6 cases)
  ffn_in<c=512,trv=16,nt=512>              mid_c512_trv16_t3, mid_c512_trv16_t17, mid_c512_trv16_t37
  ffn_in<c=512,trv=32,nt=512>              mid_c512_trv32_t3, mid_c512_trv32_t33, mid_c512_trv32_t69
  ffn_in<c=1024,trv=8,nt=512>              mid_c1024_trv8_t3, mid_c1024_trv8_t9, mid_c1024_trv8_t21, mid_c1024_trv8_t8, ... (6 cases)
  ffn_in_f32<c=2048,trv=1,nt=256>          row1_window
  ffn_in_row_kernel                        row1_hs
  ffn_out<c=128,nw=4>                      mid_c128_trv16_t3, mid_c128_trv16_t17, mid_c128_trv16_t37, mid_c128_trv32_t3, ... (9 cases)
  ffn_out<c=256,nw=4>                      mid_c256_trv8_t3, mid_c256_trv8_t9, mid_c256_trv8_t21, mid_c256_trv16_t3, ... (12 cases)
  ffn_out<c=512,nw=4>                      mid_c512_trv8_t3, mid_c512_trv8_t9, mid_c512_trv8_t21, mid_c512_trv8_t40, ... (12 cases)
  ffn_out<c=1024,nw=8>                     mid_c1024_trv8_t3, mid_c1024_trv8_t9, mid_c1024_trv8_t21, mid_c1024_trv8_t8, ... (6 cases)
  mixer_rows_kernel colfix=1               mx_r_16x256, mx_r_17x1024, mx_r_40x512, mx_r_256x256
  mixer_rows_kernel colfix=0               mx_r_16x768, mx_r_20x1280, mx_r_16x2048
  block_mixer_kernel scalar statistics     mx_s_3x30
  block1d<c=128> persistent walk           b1_c128_t229_walk3, b1_c128_t224_walk2
  vv_block_mid in place                    mid_c128_trv32_t69_inplace, mid_c256_trv16_t37_inplace, mid_c512_trv8_t21_inplace, mid_c1024_trv8_t21_inplace
"""
import ctypes as C
import functools
import os
import sys
import time
import zlib

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_mfma_gemm import NAN, _accumulate, _lib, _need_gpu, _rel, _same_bits, _steps16, bf16_round64, built_kernels, instantiations_of, \
    tile_row_errors

EPS = 1e-5
CALL_LIMIT_S = 20.0        # a call that has not finished by then fails its case (the kernels take microseconds)
FLOOR_HEADROOM = 8.0
FAULT_MARGIN = 10.0
PARAMS = ("gamma", "ffn_gamma", "norm_w", "ffn_norm_w", "dw_w", "dw_b", "w1", "b1", "w2", "b2")

# One pair of constants per class: the first is held for the global and the worst-tile figure, the second for the worst-row figure.  Faults
# (a), (b) and (e) are caught by the tile figure, (c) and (d) by the row figure, so each constant answers to the faults of its own figure.
# Chosen from the arithmetic, then checked against both conditions on the CPU (test_bars_sit_between_floor_and_faults); never from what the
# device gives.
#   y, hist   fp32 arithmetic only: a sum of squares over C <= 2048 channels (error <= sqrt(C) 2^-24 = 2.7e-6 of the statistic, half of that on
#             rsqrt), rsqrtf (1 ulp), a 7-term FMA chain and two multiplies: a few 2^-24 per element, 1e-6 at the worst.  1e-5 leaves the device
#             another summation order.  The faults of this path change elements by percents: (e) costs its tile >= 3e-2, (c) its row >= 1.5e-1.
#   hid       Tile: one bf16 step (2^-8 relative) on the few hidden values whose rounding flips; a flip on the largest element of a 3-row edge
#             tile (96 values, peak / rms ~ 2.5) costs 2^-8 x 2.5 / sqrt(96) = 1e-3, and a flipped FFN input (below) adds its row's flips.  A
#             dropped step of the first GEMM costs a 16-row tile sqrt(16 / C) of the pre-activation before GELU: 3.5e-1 at C = 128, 1.25e-1 at
#             C = 1024 (an 8-row workgroup at TRV = 8 holds half a tile: 1 / sqrt(2) of it, still 9 x the bar).  So 1.5e-2 at C = 128, 1.2e-2 at
#             256 / 512, 8e-3 at 1024, where the window is narrowest.
#             Row: the fp32 prologue flips the bf16 rounding of about 2e-5 of the FFN inputs (rsqrtf and the device's summation order flip
#             others than torch does).  One flipped input a_j moves every pre-activation of its row by 2^-8 |a_j w_nj| ~ 2^-8 |a_j| / sqrt(C) of
#             their rms, that is |a_j| / sqrt(C) of a bf16 rounding step: a 4-sigma input at C = 128 flips the rounding of a third of the row's
#             hidden values, each by one step (2^-8 relative at the bottom of a binade, 0.7 of that on average): sqrt(0.35) x 2^-8 x 0.7 =
#             1.6e-3, two such inputs in one row 2.3e-3 -> 2.5e-2; half of that from C = 256 on (|a_j| / sqrt(C) falls): 1.2e-2.  No listed fault
#             is the row figure's to catch here.
#   branch    Tile: the hidden flips arrive through W2 (sqrt(flipped share) x 2^-8 x 0.7 of the row's branch) and a 16 x 16 tile holds 16 rows
#             of which one or two are such rows: 1/4 .. 1/3 of the row figure, unless T cuts the tile to a single row.  A dropped step of the
#             second GEMM costs its tile sqrt(16 / 4C) of the product: 1.8e-1 at C = 128 .. 6.2e-2 at C = 1024 -> 9e-3 / 7e-3 / 4.5e-3 / 4e-3
#             (C = 512 and 1024 are the narrow ones: a tenth of the cheapest dropped step is 6.1e-3 and 5.4e-3).  vv_block1d: C = 128 is the
#             hard one, a dropped step of its first GEMM in one hidden block of 512 costs the branch tile 8.4e-2: 7e-3.
#             Row: as hid's row figure, over the branch instead: 2.5e-2 at C = 128 (vv_block1d, whose row figure also answers to fault (c),
#             >= 4e-1: 3e-2), 1.5e-2 at 256, 1e-2 above.
#   out       the same error over a larger value: the branch bars, so that nothing passes `out` that fails `branch` by size alone.
#   row1      the one-row stage against RowNet's fp64 reference with the FFN input rounded as the kernel rounds it (not rounded for the
#             mixer-as-own-launch mode, whose GEMV takes fp32 rows): a flipped input at C = 2048 moves the branch by 2^-8 x 3 / sqrt(2048) =
#             2.6e-4, and block 1's history is block 0's output normalised, so it inherits that.  2e-3; a history off by one row or an hs
#             built from the wrong taps is an error of order one.
BAR = {("mixer", "y"): (1e-5, 1e-5), ("mixer", "hist"): (1e-5, 1e-5),
       ("block1d", "branch"): (7e-3, 3e-2), ("block1d", "out"): (7e-3, 3e-2), ("block1d", "hist"): (1e-5, 1e-5),
       ("mid", "y"): (1e-5, 1e-5), ("mid", "hist"): (1e-5, 1e-5),
       ("mid", "hid", 128): (1.5e-2, 2.5e-2), ("mid", "hid", 256): (1.2e-2, 1.2e-2), ("mid", "hid", 512): (1.2e-2, 1.2e-2), ("mid", "hid", 1024): (8e-3, 1.2e-2),
       ("mid", "branch", 128): (9e-3, 2.5e-2), ("mid", "branch", 256): (7e-3, 1.5e-2), ("mid", "branch", 512): (4.5e-3, 1e-2), ("mid", "branch", 1024): (4e-3, 1e-2),
       ("mid", "out", 128): (9e-3, 2.5e-2), ("mid", "out", 256): (7e-3, 1.5e-2), ("mid", "out", 512): (4.5e-3, 1e-2), ("mid", "out", 1024): (4e-3, 1e-2),
       ("row1", "out"): (2e-3, 2e-3), ("row1", "state"): (2e-3, 2e-3)}
FAULT_FIGURE = {"a": 0, "b": 0, "e": 0, "c": 1, "d_hist": 1, "d_next": 1}      # 0: the tile constant answers to the fault, 1: the row constant
# Operands are drawn from a seed per (family, T, C).  Where the stand-in's own bf16 flips on the first draw leave no room between the two
# conditions, another draw is taken (the faults and the factors stay): {key: salt}
# ("mid", 21, 1024): the first draw's stand-in flips one of the largest hidden values of a 4-row edge tile (hid tile floor 1.58e-3, x 8 = 1.26e-2)
# where fault (b) / 10 is 1.0e-2 .. 1.3e-2 for the class
# At C = 1024 the window is narrow for every draw (over five draws per shape the stand-in's hid tile floor ran from 2e-5 to 1.7e-3 and fault (a)
# from 3.9e-2 to 8.3e-2), so these shapes use the draw with the most room on both sides
SEED_SALT = {("mid", 21, 1024): 1, ("mid", 64, 1024): 2, ("mid", 8, 1024): 1, ("mid", 9, 1024): 4}

TUNE_DEFAULTS = {"mixer_rows": 1, "block1d_blocks": 256, "convffn_rows512": 8, "convffn_rows256": 16, "convffn_rows128": 32, "convffn_t1": 1,
                 "convffn_t1hs": 1}
_LEDGER = dict(TUNE_DEFAULTS)       # the value each hook was last set to by this file


class _tuned:
    def __init__(self, hooks):
        self.hooks = hooks

    def _set(self, key, v):
        L, l = _lib()[:2]
        assert key in TUNE_DEFAULTS
        L.check(l.vv_tune(key.encode(), v), "vv_tune")
        _LEDGER[key] = v

    def __enter__(self):
        for key, v in self.hooks.items():
            self._set(key, v)

    def __exit__(self, *exc):
        for key in self.hooks:
            self._set(key, TUNE_DEFAULTS[key])


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def _sliced(tr, cs):
    return f"mixer_sliced<tr={tr},cs={cs}>"


def _rows(tr, colfix):
    return f"mixer_rows<tr={tr},colfix={colfix}>"


def _b1d(c, grid):
    return f"block1d<c={c}> grid={grid}"


def _ffn_in(c, trv):
    return f"ffn_in<c={c},trv={trv},nt={512 if c in (512, 1024) else 256}>"


def _ffn_out(c):
    return f"ffn_out<c={c},nw={8 if c == 1024 else 4}>"


def _mid(c, trv):
    return _ffn_in(c, trv) + " + " + _ffn_out(c)


class Case:
    """One sequence of calls on one history buffer.  fam: mixer | block1d | mid; route: what the streaming calls of T rows must report;
    route_stateless: what the closing stateless call must report (the same unless given); tr: rows per workgroup of the kernel the case is
    named for (where fault (c) and (b) are put); shorts: the two short streaming calls; inplace: vv_block_mid with out = start of ws."""

    def __init__(self, cid, fam, T, Cc, route, tr, route_stateless=None, hooks=None, inplace=False, note=""):
        self.id, self.fam, self.T, self.C, self.route, self.tr, self.hooks, self.inplace, self.note = cid, fam, T, Cc, route, tr, dict(hooks or {}), inplace, note
        self.route_stateless = route_stateless or route
        self.shorts = {"mixer": (2, 4), "block1d": (1, 4), "mid": (4, 5)}[fam]
        assert T not in self.shorts

    @property
    def calls(self):
        """(rows, streaming, entry point) of the sequence"""
        short = "mixer" if self.fam == "block1d" else self.fam
        return [(self.T, True, self.fam), (self.shorts[0], True, short), (self.shorts[1], True, short), (self.T, True, self.fam), (self.T, False, self.fam)]

    def bar(self, q):
        return BAR[(self.fam, q, self.C)] if (self.fam, q, self.C) in BAR else BAR[(self.fam, q)]

    @property
    def quantities(self):
        return {"mixer": ("y", "hist"), "block1d": ("branch", "out", "hist"), "mid": ("y", "hid", "branch", "out", "hist")}[self.fam]

    @property
    def data_key(self):      # everything the VALUES depend on: hooks and buffer placement are not part of it
        return (self.fam, self.T, self.C)


MID_DEFAULT_TRV = {128: 32, 256: 16, 512: 8, 1024: 8}
MID_FRAME_T = {512: (40, 256), 256: (200, 256), 1024: (8, 64), 128: (800, 1024)}      # the frame's own T, the largest accepted T


def _cases():
    cs = []

    def add(*a, **kw):
        cs.append(Case(*a, **kw))

    # ---- vv_block_mixer, sliced kernel ----
    add("mx_s_1x2048", "mixer", 1, 2048, _sliced(1, 64), 1, note="one row")
    add("mx_s_5x96", "mixer", 5, 96, _sliced(5, 64), 5, note="two slices, the second half-filled")
    add("mx_s_3x30", "mixer", 3, 30, _sliced(3, 32), 3, note="C % 4 != 0 (scalar statistics), CS = 32 with 30 live channels")
    add("mx_s_33x48", "mixer", 33, 48, _sliced(32, 64), 32, note="two row tiles, history rows renormalised from outside tile 0")
    add("mx_s_70x64", "mixer", 70, 64, _sliced(32, 64), 32, note="three row tiles")
    add("mx_s_15x256", "mixer", 15, 256, _sliced(15, 64), 15, note="one row under the rows kernel's threshold")
    add("mx_s_40x512_rows0", "mixer", 40, 512, _sliced(32, 64), 32, hooks={"mixer_rows": 0}, note="the rows kernel switched off")
    # ---- vv_block_mixer, rows kernel ----
    add("mx_r_16x256", "mixer", 16, 256, _rows(8, 1), 8, note="smallest T")
    add("mx_r_17x1024", "mixer", 17, 1024, _rows(8, 1), 8, note="one-row last tile")
    add("mx_r_40x512", "mixer", 40, 512, _rows(8, 1), 8)
    add("mx_r_256x256", "mixer", 256, 256, _rows(8, 1), 8, note="largest T")
    add("mx_r_16x768", "mixer", 16, 768, _rows(8, 0), 8, note="colfix = 0, three partial slots")
    add("mx_r_20x1280", "mixer", 20, 1280, _sliced(20, 64), 4, route_stateless=_rows(4, 0), note="TRr = 4, stateless only: streaming takes the sliced kernel")
    add("mx_r_16x2048", "mixer", 16, 2048, _sliced(16, 64), 2, route_stateless=_rows(2, 0), note="the smallest TRr a call reaches (2), stateless only")
    # ---- vv_block1d ----
    for c in (32, 64, 128):
        for T in (32, 33, 37, 45, 70):
            add(f"b1_c{c}_t{T}", "block1d", T, c, _b1d(c, -(-T // 32)), 32)
    add("b1_c128_t229_walk3", "block1d", 229, 128, _b1d(128, 3), 32, hooks={"block1d_blocks": 3}, note="persistent walk: 8 tiles walked 3 / 3 / 2")
    add("b1_c128_t224_walk2", "block1d", 224, 128, _b1d(128, 2), 32, hooks={"block1d_blocks": 2}, note="persistent walk: 7 full tiles walked 4 / 3")
    # ---- vv_block_mid: every (C, TRV) instantiation ----
    for c, trvs in ((128, (16, 32)), (256, (8, 16, 32)), (512, (8, 16, 32)), (1024, (8,))):
        for trv in trvs:
            dflt = trv == MID_DEFAULT_TRV[c]
            hooks = {} if (dflt or c == 1024) else {f"convffn_rows{c}": trv}
            for T in (3, trv + 1, 2 * trv + 5) + (MID_FRAME_T[c] if dflt else ()):
                add(f"mid_c{c}_trv{trv}_t{T}", "mid", T, c, _mid(c, trv), trv, hooks=hooks)
            if dflt:
                add(f"mid_c{c}_trv{trv}_t{2 * trv + 5}_inplace", "mid", 2 * trv + 5, c, _mid(c, trv), trv, inplace=True, note="out = start of ws")
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
ROW1_MODES = {"hs": {"convffn_t1": 1, "convffn_t1hs": 1}, "window": {"convffn_t1": 1, "convffn_t1hs": 0}, "mixer": {"convffn_t1": 0, "convffn_t1hs": 1}}
ROW1_KERNEL = {"hs": "ffn_in_row_kernel", "window": "ffn_in_f32<c=2048,trv=1,nt=256>", "mixer": "block_mixer_kernel"}

# the kernels of the three units this file is about: what the object files must hold, and the rows of the docstring's table
FFN_IN = [_ffn_in(c, t) for c, ts in ((128, (16, 32)), (256, (8, 16, 32)), (512, (8, 16, 32)), (1024, (8,))) for t in ts] + [ROW1_KERNEL["window"]]
FFN_OUT = [_ffn_out(c) for c in (128, 256, 512, 1024)]
BLOCK1D = [f"block1d<c={c}>" for c in (32, 64, 128)]
PLAIN = {"vv_kernels.hip": ["block_mixer_kernel", "mixer_rows_kernel"], "vv_convffn.hip": ["ffn_in_row_kernel"]}
PATHS = ["mixer_rows_kernel colfix=1", "mixer_rows_kernel colfix=0", "block_mixer_kernel scalar statistics", "block1d<c=128> persistent walk",
         "vv_block_mid in place"]


def kernels_of(case):
    """the table rows a case reaches with the calls whose route it asserts"""
    out = set()
    for r in {case.route, case.route_stateless}:
        if r.startswith("mixer_sliced"):
            out.add("block_mixer_kernel")
            if case.C % 4:
                out.add("block_mixer_kernel scalar statistics")
        elif r.startswith("mixer_rows"):
            out |= {"mixer_rows_kernel", "mixer_rows_kernel colfix=" + r[-2]}
        elif r.startswith("block1d"):
            out.add(r.split(" ")[0])
            if int(r.split("grid=")[1]) < -(-case.T // 32):
                out.add("block1d<c=128> persistent walk")
        else:
            out |= set(r.split(" + "))
            if case.inplace:
                out.add("vv_block_mid in place")
    if case.fam == "block1d":
        out.add("block_mixer_kernel")                     # its short calls
    return out


def reached():
    got = {}
    for c in CASES:
        for k in kernels_of(c):
            got.setdefault(k, []).append(c.id)
    for mode, k in ROW1_KERNEL.items():
        got.setdefault(k, []).append("row1_" + mode)
    return got


def kernel_table():
    got, lines = reached(), []
    for k in PLAIN["vv_kernels.hip"] + BLOCK1D + FFN_IN + PLAIN["vv_convffn.hip"] + FFN_OUT + PATHS:
        ids = got.get(k, [])
        lines.append(f"  {k:<40} {', '.join(ids[:4])}" + (f", ... ({len(ids)} cases)" if len(ids) > 4 else ""))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# operands, the fp64 reference and the fp32 stand-in (CPU)
# ---------------------------------------------------------------------------------------------------------------
def make_params(Cc, g):
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(gamma=r(Cc, sc=0.5), ffn_gamma=r(Cc, sc=0.5), norm_w=1 + r(Cc, sc=0.1), ffn_norm_w=1 + r(Cc, sc=0.1), dw_w=r(Cc, 7, sc=0.3), dw_b=r(Cc, sc=0.1),
                w1=(r(4 * Cc, Cc) / Cc ** 0.5).bfloat16(), b1=r(4 * Cc, sc=0.1), w2=(r(Cc, 4 * Cc) / (4 * Cc) ** 0.5).bfloat16(), b2=r(Cc, sc=0.1))


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    fam, T, Cc = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) + SEED_SALT.get(key, 0))
    p = make_params(Cc, g)
    if fam == "mixer":
        for k in ("w1", "b1", "w2", "b2", "ffn_gamma", "ffn_norm_w"):
            del p[k]
    return p, g.get_state()


def _rms(x, w):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) * w


def ref_block_fp64(p, x, hist, ffn=True, round_act=True):
    """Block1D.forward in plain fp64.  hist: the 6 normalised rows in front of x, or None for a stateless call (zero left context, nothing
    stored).  Returns y, hid, out (None without ffn) and the new history (None when stateless).  round_act=False leaves both activations
    unrounded (only to compare this function with the ref() closures of test_hip_parity.py, which never round)."""
    d = {k: v.double() for k, v in p.items()}
    x = x.double()
    T = x.shape[0]
    xn = _rms(x, d["norm_w"])
    seq = torch.cat([hist.double() if hist is not None else torch.zeros(6, x.shape[1], dtype=torch.float64), xn])
    y = x + d["gamma"] * (d["dw_b"] + sum(d["dw_w"][:, k] * seq[k: k + T] for k in range(7)))
    res = dict(y=y, hid=None, out=None, hist=seq[-6:] if hist is not None else None)
    if ffn:
        a = _rms(y, d["ffn_norm_w"])
        a = bf16_round64(a) if round_act else a
        z = a @ d["w1"].t() + d["b1"]
        h = 0.5 * z * (1 + torch.erf(z * 0.70710678118654752440))
        res["hid"] = h = bf16_round64(h) if round_act else h
        res["out"] = y + d["ffn_gamma"] * (h @ d["w2"].t() + d["b2"])
    return res


def _gemm16(a, w, drop=None):
    """fp32 a @ w.T accumulated in 16-wide K steps; drop = (rows, cols, step): that step left out of that tile"""
    P = _steps16(a, w)
    z = _accumulate(P)
    if drop is not None:
        rs, cs, s = drop
        z[rs, cs] = _accumulate(P, s, rs, cs)
    return z


def stand_in(p, x, hist, ffn=True, fault=None):
    """The same block as the kernels compute it, in torch fp32: fp32 prologue, bf16 where the kernels round, 16-wide K steps.  fault: None or
    ("w2step", rows, cols, step) | ("w1step", rows, cols, step) | ("halo", t0, rows) (the row in front of t0 replaced by the one before it, for
    the conv of rows t0 .. t0 + rows) | ("shift",) (the stored history one row late) | ("taps", c0) (the taps of the newest row and the one before it swapped in channels c0 .. c0 + 3)."""
    f = {k: v.float() for k, v in p.items()}
    kind = fault[0] if fault else None
    T, Cc = x.shape
    xn = _rms(x, f["norm_w"])
    seq = torch.cat([hist.float() if hist is not None else torch.zeros(6, Cc), xn])
    dw = f["dw_w"]
    if kind == "taps":
        dw = dw.clone()
        dw[fault[1]: fault[1] + 4, 5], dw[fault[1]: fault[1] + 4, 6] = f["dw_w"][fault[1]: fault[1] + 4, 6], f["dw_w"][fault[1]: fault[1] + 4, 5]
    conv = lambda s, t0, n: f["dw_b"] + sum(dw[:, k] * s[t0 + k: t0 + k + n] for k in range(7))
    y = x + f["gamma"] * conv(seq, 0, T)
    if kind == "halo":
        t0, n = fault[1], min(fault[2], T - fault[1])
        s2 = seq.clone()
        s2[t0 + 5] = seq[t0 + 4]                             # window row t0 - 1 sits at seq[t0 - 1 + 6]
        y[t0: t0 + n] = x[t0: t0 + n] + f["gamma"] * conv(s2, t0, n)
    new_hist = None
    if hist is not None:
        new_hist = seq[-7:-1] if kind == "shift" else seq[-6:]
    res = dict(y=y, hid=None, out=None, hist=new_hist)
    if ffn:
        a = _rms(y, f["ffn_norm_w"]).bfloat16().float()
        z = _gemm16(a, p["w1"], fault[1:] if kind == "w1step" else None) + f["b1"]
        h = (0.5 * z * (1 + torch.erf(z * 0.70710678118654752440))).bfloat16().float()
        res["hid"] = h
        res["out"] = y + f["ffn_gamma"] * (_gemm16(h, p["w2"], fault[1:] if kind == "w2step" else None) + f["b2"])
    return res


def figures(got, ref, tm=16, tn=16):
    """(global, worst tile, worst row) rel RMS and where: ((tile row, tile column), row)"""
    t, ti, r, ri = tile_row_errors(got, ref, tm, tn)
    return (_rel(got, ref), t, r), (ti, ri)


def compare(case, got, ref):
    """{quantity: ((global, tile, row), where)} of one call's results (dicts of y / hid / out / hist; absent or None: not exposed)"""
    out = {}
    num = lambda t: np.asarray(t.double() if torch.is_tensor(t) else t, dtype=np.float64)
    if got.get("y") is not None and "y" in case.quantities:
        out["y"] = figures(num(got["y"]), num(ref["y"]))
    if got.get("hid") is not None:
        out["hid"] = figures(num(got["hid"]), num(ref["hid"]), 16, 32)
    if got.get("out") is not None:
        out["branch"] = figures(num(got["out"]) - num(ref["y"]), num(ref["out"]) - num(ref["y"]))
        out["out"] = figures(num(got["out"]), num(ref["out"]))
    if got.get("hist") is not None:
        g, h = num(got["hist"]), num(ref["hist"])
        rows = np.sqrt(((g - h) ** 2).sum(1) / ((h ** 2).sum(1) + 1e-300))
        rows[(h ** 2).sum(1) == 0] = np.sqrt(((g - h) ** 2).sum(1))[(h ** 2).sum(1) == 0]          # a row that must still be zero
        out["hist"] = ((_rel(g, h) if h.any() else float(rows.max()), float(rows.max()), float(rows.max())), ((0, 0), int(rows.argmax())))
    return out


@functools.lru_cache(maxsize=None)
def _sequence_of(key):
    """[(x, streaming, fp64 reference results)] of the five calls of a case's operands, the reference's own history carried"""
    fam, T, Cc = key
    p, state = _operands_of(key)
    g = torch.Generator()
    g.set_state(state)
    case = next(c for c in CASES if c.data_key == key)
    hist, seq = torch.zeros(6, Cc, dtype=torch.float64), []
    for rows, streaming, entry in case.calls:
        x = torch.randn(rows, Cc, generator=g)
        ref = ref_block_fp64(p, x, hist if streaming else None, ffn=(fam != "mixer") and entry != "mixer")
        if streaming:
            hist = ref["hist"]
        seq.append((x, streaming, ref))
    return seq


def _mixer_only(p):
    return {k: p[k] for k in ("gamma", "norm_w", "dw_w", "dw_b")}


@functools.lru_cache(maxsize=None)
def _expect_of(key, tr):
    """(floor {quantity: (global, tile, row)} of the fp32 stand-in over the five calls, its own history carried; {fault: (quantity, cost)})"""
    fam, T, Cc = key
    case = next(c for c in CASES if c.data_key == key)
    p, _ = _operands_of(key)
    seq = _sequence_of(key)
    floor, hist = {}, torch.zeros(6, Cc)
    for (x, streaming, ref), (_, _, entry) in zip(seq, case.calls):
        ffn = fam != "mixer" and entry != "mixer"
        got = stand_in(p if ffn else _mixer_only(p), x, hist if streaming else None, ffn=ffn)
        if streaming:
            hist = got["hist"]
        if fam == "block1d":
            got["y"] = None
        for q, (fig, _) in compare(case, got, ref).items():
            if q in case.quantities:
                floor[q] = tuple(max(a, b) for a, b in zip(floor.get(q, (0, 0, 0)), fig))
    # faults, in the first call (x0, zero history) and for (d) the second
    x0, _, ref0 = seq[0]
    x1, _, ref1 = seq[1]
    z6 = torch.zeros(6, Cc)
    ffn = fam != "mixer"
    yq = "branch" if fam == "block1d" else "y"

    def fig_of(fault, q, which, n):
        """the figure over the first n rows alone (the block is causal, so they are the full call's rows; the faulted tile or row lies inside
        them, and the worst of fewer tiles is no larger: the cost is never overstated)"""
        got = stand_in(p, x0[:n], z6, ffn=ffn, fault=fault)
        if fam == "block1d":
            got["y"] = None
        return compare(case, got, {k: (v[:n] if k != "hist" and v is not None else v) for k, v in ref0.items()})[q][0][which]

    cost = {}
    if ffn:
        S2, S1 = 4 * Cc // 16, Cc // 16
        rs, cs = slice(0, min(16, T)), slice(0, 16)
        cost["a"] = ("branch", min(fig_of(("w2step", rs, cs, s), "branch", 1, 16) for s in {0, S2 // 2, S2 - 1}))
        cost["b"] = ("hid" if fam == "mid" else "branch", min(fig_of(("w1step", rs, slice(0, 32), s), "hid" if fam == "mid" else "branch", 1, 16) for s in {0, S1 // 2, S1 - 1}))
    if T > tr:
        cost["c"] = (yq, fig_of(("halo", tr, tr), yq, 2, 2 * tr))
    cost["e"] = (yq, fig_of(("taps", 4 * ((Cc // 4) // 2)), yq, 1, 16))
    # (d): the first call stores its history one row late; the history figure sees it at once, y (branch) in the next call
    late = stand_in(p, x0, z6, ffn=False, fault=("shift",))["hist"]
    cost["d_hist"] = ("hist", compare(case, dict(hist=late), ref0)["hist"][0][2])
    short_ffn = ffn and case.calls[1][2] != "mixer"
    nxt = stand_in(p if short_ffn else _mixer_only(p), x1, late, ffn=short_ffn)
    if fam == "block1d":                                     # its short call is a mixer call: the wrong rows show in that call's y
        cost["d_next"] = ("y", figures(nxt["y"].double().numpy(), ref1["y"].numpy())[0][2])
    else:
        cost["d_next"] = (yq, compare(case, nxt, ref1)[yq][0][2])
    return floor, cost


def expect(case):
    return _expect_of(case.data_key, case.tr)


# ---------------------------------------------------------------------------------------------------------------
# CPU-only guards
# ---------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_ref_closures_of_the_parity_suite():
    """Guards the reference (CPU only): with both roundings switched off it is the ref() closure of test_block1d_single_launch_vs_torch /
    test_block_mid_two_launches_vs_torch and the inline reference of test_block_mixer_vs_torch, recomputed in fp64, to 1e-12 - over a
    streaming call with a non-zero history and a stateless one."""
    g = torch.Generator().manual_seed(5)
    Cc, T = 64, 11
    p = make_params(Cc, g)
    d = {k: v.double() for k, v in p.items()}

    def rms(x, w): return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) * w

    def ref(x, hist):                                        # the closure of test_hip_parity.py, on fp64 tensors
        xn = rms(x, d["norm_w"])
        seq = torch.cat([hist, xn])
        s = d["dw_b"] + sum(d["dw_w"][:, k] * seq[k: k + x.shape[0]] for k in range(7))
        x1 = x + d["gamma"] * s
        h = torch.nn.functional.gelu(rms(x1, d["ffn_norm_w"]) @ d["w1"].T + d["b1"])
        return x1, x1 + d["ffn_gamma"] * (h @ d["w2"].T + d["b2"]), seq[-6:]

    x, hist = torch.randn(T, Cc, generator=g), torch.randn(6, Cc, generator=g).double()
    for h_in in (hist, None):
        y, out, new = ref(x.double(), h_in if h_in is not None else torch.zeros(6, Cc, dtype=torch.float64))
        got = ref_block_fp64(p, x, h_in, round_act=False)
        assert _rel(got["y"].numpy(), y.numpy()) < 1e-12 and _rel(got["out"].numpy(), out.numpy()) < 1e-12
        assert (got["hist"] is None) if h_in is None else _rel(got["hist"].numpy(), new.numpy()) < 1e-12
        mix = ref_block_fp64(_mixer_only(p), x, h_in, ffn=False)
        assert torch.equal(mix["y"], got["y"]) and mix["out"] is None
    # and the two roundings it adds are bf16 roundings, no more: ~ 2^-9 / sqrt(3) of the branch each
    y, out, _ = ref(x.double(), hist)
    e = _rel((ref_block_fp64(p, x, hist)["out"] - y).numpy(), (out - y).numpy())
    assert 2e-4 < e < 6e-3, e


def test_stand_in_without_fault_is_the_reference_in_fp32():
    """the stand-in's faults are what move it: without one it stays within fp32 / bf16-flip distance of the reference, and each fault moves
    only what it should (a dropped step of the second GEMM leaves y and hid alone, a shifted history leaves the call's own outputs alone)"""
    g = torch.Generator().manual_seed(6)
    p = make_params(64, g)
    x, hist = torch.randn(40, 64, generator=g), torch.randn(6, 64, generator=g)
    ref, got = ref_block_fp64(p, x, hist), stand_in(p, x, hist)
    assert _rel(got["y"].double().numpy(), ref["y"].numpy()) < 1e-6 and _rel(got["out"].double().numpy(), ref["out"].numpy()) < 1e-3
    a = stand_in(p, x, hist, fault=("w2step", slice(0, 16), slice(16, 32), 3))
    assert torch.equal(a["y"], got["y"]) and torch.equal(a["hid"], got["hid"]) and torch.equal(a["hist"], got["hist"])
    changed = (a["out"] != got["out"])
    assert changed[:16, 16:32].any() and not changed[16:].any() and not changed[:, :16].any() and not changed[:, 32:].any()
    s = stand_in(p, x, hist, fault=("shift",))
    assert torch.equal(s["out"], got["out"]) and torch.equal(s["hist"][1:], got["hist"][:-1])
    h = stand_in(p, x, hist, fault=("halo", 32, 32))
    assert torch.equal(h["y"][:32], got["y"][:32]) and not torch.equal(h["y"][32:38], got["y"][32:38]) and torch.equal(h["y"][38:], got["y"][38:])


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_faults(cid):
    """Both conditions on every bar of the case (CPU only): at least 8 x the fp32 stand-in's own error against the fp64 reference over the
    case's five calls (global, worst tile, worst row), at most a tenth of what each fault costs the figure meant to catch it."""
    case = CASES[CASE_IDS.index(cid)]
    floor, cost = expect(case)
    for q in case.quantities:
        bt, br = case.bar(q)
        print(f"{cid}: {q:<6} bars {bt:.1e} / {br:.1e}  floor global {floor[q][0]:.2e} tile {floor[q][1]:.2e} row {floor[q][2]:.2e}")
        assert bt >= FLOOR_HEADROOM * max(floor[q][:2]) and br >= FLOOR_HEADROOM * floor[q][2], (cid, q, case.bar(q), floor[q])
    for name, (q, c) in cost.items():
        bar = (BAR[("mixer", "y")] if (case.fam == "block1d" and q == "y") else case.bar(q))[FAULT_FIGURE[name]]
        print(f"{cid}: fault {name:<6} costs {q} {('tile', 'row')[FAULT_FIGURE[name]]} {c:.2e} (bar {bar:.1e})")
        assert bar <= c / FAULT_MARGIN, (cid, name, q, bar, c)
    want = {"d_hist", "d_next", "e"} | ({"a", "b"} if case.fam != "mixer" else set()) | ({"c"} if case.T > case.tr else set())
    assert set(cost) == want


def test_docstring_table_is_current():
    """the kernel -> case table of the docstring is the one the parametrisation generates, and every kernel and path has a case"""
    assert kernel_table() in __doc__
    got = reached()
    for k in PLAIN["vv_kernels.hip"] + BLOCK1D + FFN_IN + PLAIN["vv_convffn.hip"] + FFN_OUT + PATHS:
        assert got.get(k), f"no case reaches {k}"


def test_built_units_hold_exactly_the_kernels_the_cases_reach(tmp_path):
    """The code objects of vv_block1d.hip and vv_convffn.hip hold the instantiations of block1d_kernel, ffn_in_kernel and ffn_out_kernel that the
    cases' route assertions name, and no other; block_mixer_kernel, mixer_rows_kernel and ffn_in_row_kernel are there by name (CPU only: reads
    the symbol tables of the object files build() left)."""
    got = reached()
    names = {"ffn_in_kernel": lambda c, trv, hf32, nt: f"ffn_in{'_f32' if hf32 else ''}<c={c},trv={trv},nt={nt}>",
             "ffn_out_kernel": lambda c, nw: f"ffn_out<c={c},nw={nw}>"}
    cf = built_kernels("vv_convffn.hip", tmp_path, plain=True)
    built = instantiations_of(cf, names)
    assert built == set(FFN_IN + FFN_OUT), sorted(built ^ set(FFN_IN + FFN_OUT))
    assert built == {k for k in got if k.startswith(("ffn_in<", "ffn_in_f32<", "ffn_out<"))}
    b1 = instantiations_of(built_kernels("vv_block1d.hip", tmp_path), {"block1d_kernel": lambda c: f"block1d<c={c}>"})
    assert b1 == set(BLOCK1D) == {k for k in got if k.startswith("block1d<") and " " not in k}
    assert "ffn_in_row_kernel" in [k for k, _ in cf]
    kk = [k for k, _ in built_kernels("vv_kernels.hip", tmp_path, plain=True)]
    assert kk.count("block_mixer_kernel") == 1 and kk.count("mixer_rows_kernel") == 1


# ---------------------------------------------------------------------------------------------------------------
# the calls: routes on the host, then the device with guards
# ---------------------------------------------------------------------------------------------------------------
_FAKE = {name: 0x10000000 * (i + 1) for i, name in enumerate(("x", "out", "hist", "ws") + PARAMS)}


def _block(ptr, hist):
    L = _lib()[0]
    b = L.Block()
    for k in PARAMS:
        setattr(b, k, ptr[k])
    b.hist = hist or None
    return b


def route_of(entry, ptr, rows, Cc, hist, want_rc=0):
    """the route query of one entry point; ptr: {name: address}; hist: address or 0"""
    L, l = _lib()[:2]
    name = C.create_string_buffer(128)
    if entry == "mixer":
        rc = l.vv_block_mixer_route(ptr["x"], ptr["out"], rows, Cc, ptr["norm_w"], ptr["dw_w"], ptr["dw_b"], ptr["gamma"], hist or None, name, 128)
    elif entry == "block1d":
        rc = l.vv_block1d_route(C.byref(_block(ptr, hist)), L.VV_BF16, ptr["x"], ptr["out"], rows, Cc, name, 128)
    else:
        rc = l.vv_block_mid_route(C.byref(_block(ptr, hist)), L.VV_BF16, ptr["x"], ptr["out"], ptr["ws"], rows, Cc, name, 128)
    assert rc == want_rc, (entry, rows, Cc, rc, l.vv_last_error())
    return name.value.decode()


def _want_route(case, i):
    rows, streaming, entry = case.calls[i]
    if rows != case.T:
        return None
    return case.route if streaming else case.route_stateless


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_call_on_the_host(cid):
    """The route queries need no device: every call of every case (16-byte aligned stand-in addresses, nothing is dereferenced) reports the
    kernel the case is named for, here on the CPU too, and the tune state is back at its defaults afterwards."""
    case = CASES[CASE_IDS.index(cid)]
    ptr = {**_FAKE, **({"out": _FAKE["ws"]} if case.inplace else {})}
    with _tuned(case.hooks):
        for i, (rows, streaming, entry) in enumerate(case.calls):
            got = route_of(entry, ptr, rows, case.C, _FAKE["hist"] if streaming else 0)
            want = _want_route(case, i)
            assert got and (want is None or got == want), (cid, i, got, want)
    _default_routes()


def _default_routes():
    """five fixed shapes whose default routes a leaked vv_tune setting would change"""
    assert route_of("mixer", _FAKE, 40, 512, 0) == _rows(8, 1)
    assert route_of("block1d", _FAKE, 32 * 300, 128, _FAKE["hist"]) == _b1d(128, 256)
    for c in (128, 256, 512):
        assert route_of("mid", _FAKE, 40, c, _FAKE["hist"]) == _mid(c, MID_DEFAULT_TRV[c])


def test_route_refusals_match_the_calls():
    """CPU only: arguments the calls refuse are refused by the queries with the same code and text (-1 VV_E_ARG, -3 VV_E_UNSUPPORTED)"""
    L, l = _lib()[:2]
    for entry, rows, Cc, kw, rc, text in (("block1d", 8, 64, {}, -3, "not covered by the fused kernel"), ("block1d", 40, 48, {}, -3, "not covered"),
                                          ("block1d", 40, 64, {"out": _FAKE["x"] + 64}, -3, "not covered"), ("block1d", 0, 64, {}, -1, "bad args"),
                                          ("mid", 2, 256, {}, -3, "shape not covered"), ("mid", 65, 1024, {}, -3, "shape not covered"),
                                          ("mid", 257, 512, {}, -3, "shape not covered"), ("mid", 40, 512, {"w1": _FAKE["w1"] + 4}, -3, "shape not covered"),
                                          ("mid", 40, 512, {"ws": 0}, -1, "bad args"),
                                          ("mixer", 8, 64, {"out": _FAKE["x"]}, -1, "in-place"), ("mixer", 0, 64, {}, -1, "bad shape"),
                                          ("mixer", 8, 64, {"gamma": 0}, -1, "null pointer")):
        assert route_of(entry, {**_FAKE, **kw}, rows, Cc, _FAKE["hist"], want_rc=rc) == ""
        assert text in l.vv_last_error().decode(), (entry, rows, Cc, l.vv_last_error())
    name = C.create_string_buffer(8)
    assert l.vv_block_mixer_route(_FAKE["x"], _FAKE["out"], 8, 64, _FAKE["norm_w"], _FAKE["dw_w"], _FAKE["dw_b"], _FAKE["gamma"], None, name, 0) == -1


def _wait(what):
    """the device under a time limit: a call that has not finished after CALL_LIMIT_S fails the case instead of blocking the session"""
    ev = torch.cuda.Event()
    ev.record()
    end = time.monotonic() + CALL_LIMIT_S
    while not ev.query():
        assert time.monotonic() < end, f"{what}: not finished after {CALL_LIMIT_S} s"
        time.sleep(0)


def _guarded(rows, Cc, fill=None):
    """[2 + rows + 2, Cc] on the device, NaN; the middle rows hold `fill` when given.  Returns (buffer, view of the middle rows)."""
    buf = torch.full((rows + 4, Cc), NAN, device="cuda")
    if fill is not None:
        buf[2: 2 + rows] = fill
    return buf, buf[2: 2 + rows]


def _guards_intact(buf, rows):
    h = buf.cpu()
    return bool(torch.isnan(h[:2]).all() and torch.isnan(h[2 + rows:]).all())


class _State:
    """one set of device buffers for a case's sequence: parameters, the guarded history"""

    def __init__(self, case, p):
        self.dev = {k: v.cuda().contiguous() for k, v in p.items()}
        self.hist_buf, self.hist = _guarded(6, case.C, 0.0)


def run_call(case, st, p, x, rows, streaming, entry, want_route):
    """One call on the buffers of `st`: route assertion, launch, wait, guards.  Returns {y, hid, out, hist} as host tensors (None: not exposed)
    and the route."""
    L, l = _lib()[:2]
    Cc = case.C
    xd = x.cuda()
    out_buf, out = _guarded(rows, Cc)
    ptr = {k: t.data_ptr() for k, t in st.dev.items()}
    ptr["x"] = xd.data_ptr()
    hp = st.hist.data_ptr() if streaming else 0
    hist_before = st.hist_buf.cpu()
    res = dict(y=None, hid=None, out=None, hist=None)
    ws = None
    if entry == "mid":
        nb = l.vv_block_mid_ws_bytes(rows, Cc)
        ws = torch.full((nb + 512,), 0xFF, dtype=torch.uint8, device="cuda")
        ptr["ws"] = ws.data_ptr() + 256
        assert ptr["ws"] % 16 == 0
    ptr["out"] = ptr["ws"] if (case.inplace and entry == "mid") else out.data_ptr()
    route = route_of(entry, ptr, rows, Cc, hp)
    assert want_route is None or route == want_route, (case.id, rows, streaming, route, want_route)
    what = f"{case.id}: {entry} T={rows} {'streaming' if streaming else 'stateless'} [{route}]"
    if entry == "mixer":
        L.check(l.vv_block_mixer(ptr["x"], ptr["out"], rows, Cc, ptr["norm_w"], EPS, ptr["dw_w"], ptr["dw_b"], ptr["gamma"], hp or None, None), what)
    elif entry == "block1d":
        L.check(l.vv_block1d(C.byref(_block(ptr, hp)), L.VV_BF16, ptr["x"], ptr["out"], rows, Cc, EPS, None), what)
    else:
        L.check(l.vv_block_mid(C.byref(_block(ptr, hp)), L.VV_BF16, ptr["x"], ptr["out"], ptr["ws"], rows, Cc, EPS, None), what)
    _wait(what)
    # inputs
    assert _same_bits(xd.cpu(), x), f"{what}: x was written"
    for k, t in st.dev.items():
        assert _same_bits(t.cpu(), p[k]), f"{what}: parameter {k} was written"
    assert _guards_intact(st.hist_buf, 6), f"{what}: a guard row of the history was written"
    if streaming:
        res["hist"] = st.hist.cpu()
        assert torch.isfinite(res["hist"]).all(), f"{what}: the new history is not finite"
    else:
        assert _same_bits(st.hist_buf.cpu(), hist_before), f"{what}: a stateless call wrote the history"
    # outputs
    assert _guards_intact(out_buf, rows), f"{what}: a guard row of out was written"
    if ws is not None:
        h = ws.cpu()
        assert bool((h[:256] == 0xFF).all() and (h[256 + nb:] == 0xFF).all()), f"{what}: a guard byte of the workspace was written"
        body = h[256: 256 + nb]
        first = body[: rows * Cc * 4].view(torch.float32).view(rows, Cc).clone()
        res["hid"] = body[rows * Cc * 4: rows * Cc * 4 + rows * 4 * Cc * 2].view(torch.bfloat16).view(rows, 4 * Cc).float()
        assert torch.isfinite(res["hid"]).all(), f"{what}: the hidden activation in ws is not finite"
        if case.inplace:
            res["out"] = first
            assert torch.isnan(out.cpu()).all(), f"{what}: the in-place call wrote the separate out"
        else:
            res["y"], res["out"] = first, out.cpu()
    elif entry == "mixer":
        res["y"] = out.cpu()
    else:
        res["out"] = out.cpu()
    for q in ("y", "out"):
        assert res[q] is None or torch.isfinite(res[q]).all(), f"{what}: {int((~torch.isfinite(res[q])).sum())} in-range values of {q} are not finite"
    return res, route


_MEASURED = {}      # class -> [global, tile, row] maxima of this session, written by _report


def _klass(case, q):
    return (case.fam, q, case.C) if (case.fam, q, case.C) in BAR else (case.fam, q)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_conv_block_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    p, _ = _operands_of(case.data_key)
    seq = _sequence_of(case.data_key)
    states = [_State(case, p), _State(case, p)]
    fails = []
    with _tuned(case.hooks):
        for i, ((x, streaming, ref), (rows, _, entry)) in enumerate(zip(seq, case.calls)):
            pp = _mixer_only(p) if entry == "mixer" else p
            runs = []
            for st in states:
                if entry == "mixer" and case.fam != "mixer":
                    sub = _State.__new__(_State)
                    sub.dev, sub.hist_buf, sub.hist = {k: st.dev[k] for k in pp}, st.hist_buf, st.hist
                    runs.append(run_call(case, sub, pp, x, rows, streaming, entry, None))
                else:
                    runs.append(run_call(case, st, pp, x, rows, streaming, entry, _want_route(case, i)))
            (got, route), (again, _) = runs
            for q in got:
                assert (got[q] is None) == (again[q] is None) and (got[q] is None or _same_bits(got[q], again[q])), f"{cid} call {i}: two runs of the same call differ in {q}"
            if case.fam == "block1d" and entry == "mixer":
                figs = {"hist": compare(case, dict(hist=got["hist"]), ref)["hist"], "y": figures(got["y"].double().numpy(), ref["y"].numpy())}
            else:
                figs = compare(case, got, ref)
            for q, ((g, t, r), (ti, ri)) in figs.items():
                bt, br = BAR[("mixer", "y")] if (case.fam == "block1d" and q == "y") else case.bar(q)
                print(f"{cid} call {i} T={rows} {'s' if streaming else '-'} [{route}] {q:<6} bars {bt:.1e} / {br:.1e}  global {g:.3e}  worst tile {t:.3e} at {ti}  worst row {r:.3e} (row {ri})")
                if not (case.fam == "block1d" and q == "y"):
                    mx = _MEASURED.setdefault(_klass(case, q), [0.0, 0.0, 0.0, 0])
                    for j, v in enumerate((g, t, r)):
                        mx[j] = max(mx[j], v)
                    mx[3] += 1
                for name, v, bar, where in (("global", g, bt, ""), ("tile", t, bt, f" at (row tile {ti[0]}, channel tile {ti[1]})"), ("row", r, br, f" (row {ri})")):
                    if not v < bar:
                        fails.append(f"{cid} call {i} T={rows} [{route}]: {q} {name} rel RMS {v:.3e}{where} >= {bar:.1e}")
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_refusals_launch_nothing():
    """vv_block1d with fp32 weights and with T < 32, vv_block_mid with fp32 weights and with T < 3: call and route query both refuse with the
    same code, and neither the output nor the history is touched."""
    _need_gpu()
    L, l = _lib()[:2]
    Cc = 128
    p = make_params(Cc, torch.Generator().manual_seed(9))
    dev = {k: v.cuda().contiguous() for k, v in p.items()}
    ptr = {k: t.data_ptr() for k, t in dev.items()}
    x, out, hist = torch.randn(40, Cc).cuda(), torch.full((40, Cc), NAN, device="cuda"), torch.full((6, Cc), NAN, device="cuda")
    ws = torch.empty(l.vv_block_mid_ws_bytes(40, Cc), dtype=torch.uint8, device="cuda")
    ptr.update(x=x.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr())
    b = _block(ptr, hist.data_ptr())
    name = C.create_string_buffer(128)
    for wdt, T in ((L.VV_F32, 40), (L.VV_BF16, 8)):
        assert l.vv_block1d(C.byref(b), wdt, ptr["x"], ptr["out"], T, Cc, EPS, None) == -3
        assert l.vv_block1d_route(C.byref(b), wdt, ptr["x"], ptr["out"], T, Cc, name, 128) == -3
    for wdt, T in ((L.VV_F32, 40), (L.VV_BF16, 2)):
        assert l.vv_block_mid(C.byref(b), wdt, ptr["x"], ptr["out"], ptr["ws"], T, Cc, EPS, None) == -3
        assert l.vv_block_mid_route(C.byref(b), wdt, ptr["x"], ptr["out"], ptr["ws"], T, Cc, name, 128) == -3
    _wait("refusals")
    assert torch.isnan(out).all() and torch.isnan(hist).all()


# ---------------------------------------------------------------------------------------------------------------
# the one-row stage (C = 2048): RowNet of test_hip_conv_hot.py, 8 frames, three modes
# ---------------------------------------------------------------------------------------------------------------
ROW1_FRAMES = 8


@functools.lru_cache(maxsize=None)
def _row_net():
    """(the net, its fp64 reference frames without and with the FFN input rounded): built once, shared by the three modes, left unchanged"""
    from test_hip_conv_hot import RowNet

    class Rows8(RowNet):
        def __init__(self, L):
            super().__init__(L)
            g = torch.Generator().manual_seed(88)
            self.lats = self.lats + [torch.randn(1, self.LAT, generator=g) for _ in range(ROW1_FRAMES - len(self.lats))]

        def run_frames(self):
            """ROW1_FRAMES consecutive frames from zeroed state under the current tune state, conv_hot off; per frame (out row, hists, hs)"""
            L, l = self.L, self.L.load()
            lat = torch.empty(1, self.LAT, device="cuda")
            buf, wav = _guarded(1, self.C_)
            frames = []
            self.reset()
            L.check(l.vv_tune(b"conv_hot", 0), "vv_tune")
            try:
                for f in range(ROW1_FRAMES):
                    lat.copy_(self.lats[f])
                    L.check(l.vv_decoder_forward(C.byref(self.net), lat.data_ptr(), 1, 1.0, 0.0, wav.data_ptr(), self.ws.data_ptr(), None), "vv_decoder_forward")
                    _wait(f"one-row stage, frame {f}")
                    assert _guards_intact(buf, 1), f"frame {f}: a guard row of the output was written"
                    frames.append((wav[0].cpu(), [h.cpu() for h in self.hist], [h.cpu() for h in self.hs]))
            finally:
                l.vv_tune(b"conv_hot", -1)
            return frames

        def reference_frames(self, round_in):
            """RowNet.reference() for ROW1_FRAMES frames, in fp64; round_in: the FFN input rounded to bf16 once, as ffn_in_kernel and
            ffn_in_row_kernel round it (the hidden row stays fp32 on this stage)"""
            p, eps = self.p, self.EPS
            rms = lambda v, w: v * torch.rsqrt((v * v).mean() + eps) * w.double()
            stem_hist = torch.zeros(6, self.LAT, dtype=torch.float64)
            hists = [torch.zeros(6, self.C_, dtype=torch.float64) for _ in range(self.NB)]
            out = []
            for f in range(ROW1_FRAMES):
                win = torch.cat([stem_hist, self.lats[f].double()])
                stem_hist = win[1:]
                x = p["stem_w"].double() @ win.reshape(-1) + p["stem_b"].double()
                for j, b in enumerate(p["blocks"]):
                    xn = rms(x, b["norm_w"])
                    win = torch.cat([hists[j], xn[None]])
                    hists[j] = win[1:]
                    y = x + b["gamma"].double() * ((b["dw_w"].double().t() * win).sum(0) + b["dw_b"].double())
                    a = rms(y, b["ffn_norm_w"])
                    a = bf16_round64(a) if round_in else a
                    h = torch.nn.functional.gelu(b["w1"].double() @ a + b["b1"].double())
                    x = y + b["ffn_gamma"].double() * (b["w2"].double() @ h + b["b2"].double())
                hs = [(b["dw_w"].double()[:, :6].t() * hists[j]).sum(0) for j, b in enumerate(p["blocks"])]
                out.append((x, [h.clone() for h in hists], hs))
            return out

    net = Rows8(_lib()[0])
    plain = net.reference_frames(False)
    for f, old in enumerate(net.reference()):            # the first two frames of the unrounded reference are RowNet.reference()
        assert _rel(plain[f][0].numpy(), old[0].double().numpy()) < 1e-6 and _rel(plain[f][1][1].numpy(), old[1][1].double().numpy()) < 1e-6
    return net, plain, net.reference_frames(True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(ROW1_MODES))
def test_one_row_stage_vs_fp64(mode):
    """8 frames, so that the history has turned over fully and hs is built from six real rows: the output row, every block's history (per
    row) and hs, per frame, against fp64 - with the hs kernel (ffn_in_row_kernel), the window-rebuilding kernel (ffn_in_kernel<2048, 1, true>)
    and the mixer as its own launch (block_mixer_kernel at T = 1).  The first two frames of the unrounded reference are RowNet.reference()."""
    _need_gpu()
    net, plain, rounded = _row_net()
    want = plain if mode == "mixer" else rounded
    with _tuned(ROW1_MODES[mode]):
        got, again = net.run_frames(), net.run_frames()
    fails = []
    for f in range(ROW1_FRAMES):
        assert torch.equal(got[f][0], again[f][0]) and all(torch.equal(a, b) for a, b in zip(got[f][1] + got[f][2], again[f][1] + again[f][2])), f"{mode}: frame {f} differs between two runs"
        assert torch.isfinite(got[f][0]).all()
        e_out = _rel(got[f][0].double().numpy(), want[f][0].numpy())
        e_hist = max(compare(None, dict(hist=g), dict(hist=w))["hist"][0][2] for g, w in zip(got[f][1], want[f][1]))
        e_hs = max(_rel(g.double().numpy(), w.numpy()) for g, w in zip(got[f][2], want[f][2]))
        print(f"row1_{mode} frame {f}: out {e_out:.3e} (bar {BAR[('row1', 'out')][0]:.1e})  worst history row {e_hist:.3e}  hs {e_hs:.3e} (bar {BAR[('row1', 'state')][0]:.1e})")
        mo, ms = _MEASURED.setdefault(("row1", "out"), [0.0, 0.0, 0.0, 0]), _MEASURED.setdefault(("row1", "state"), [0.0, 0.0, 0.0, 0])
        mo[0], mo[2], mo[3] = max(mo[0], e_out), max(mo[2], e_out), mo[3] + 1
        ms[0], ms[2], ms[3] = max(ms[0], e_hs), max(ms[2], e_hist), ms[3] + 1
        if not e_out < BAR[("row1", "out")][0]:
            fails.append(f"{mode} frame {f}: output row rel RMS {e_out:.3e}")
        if not max(e_hist, e_hs) < BAR[("row1", "state")][0]:
            fails.append(f"{mode} frame {f}: worst history row {e_hist:.3e}, hs {e_hs:.3e}")
    assert float(got[-1][1][0][0].abs().max()) > 0, "the oldest history row is still zero after 8 frames"
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_zz_tune_state_is_back_at_its_defaults():
    """Hook hygiene: every hook this file set is back at its default by the file's own ledger, and five fixed shapes report their default
    routes, so a vv_tune setting leaked by any test above fails here."""
    _need_gpu()
    assert _LEDGER == TUNE_DEFAULTS, {k: v for k, v in _LEDGER.items() if v != TUNE_DEFAULTS[k]}
    _default_routes()
    _report()


def _report():
    """the session's largest figures per class, for the docstring and profiles/conv_block_parity.txt (written only where VV_CONV_BLOCK_PARITY_OUT says)"""
    path = os.environ.get("VV_CONV_BLOCK_PARITY_OUT")
    if not path or not _MEASURED:
        return
    with open(path, "w") as f:
        f.write(f"{torch.cuda.get_device_name(0)}: largest rel RMS against fp64 over each class's calls (tests/test_hip_conv_block.py)\n")
        f.write(f"{'class':<22} {'calls':>5} {'bar tile':>9} {'bar row':>9} {'global':>10} {'tile':>10} {'row':>10} {'bar / largest':>14}\n")
        for k in BAR:
            if k in _MEASURED:
                g, t, r, n = _MEASURED[k]
                f.write(f"{' '.join(str(s) for s in k):<22} {n:>5} {BAR[k][0]:>9.1e} {BAR[k][1]:>9.1e} {g:>10.2e} {t:>10.2e} {r:>10.2e} "
                        f"{min(BAR[k][0] / max(g, t, 1e-300), BAR[k][1] / max(r, 1e-300)):>14.1f}\n")


if __name__ == "__main__":
    if "--table" in sys.argv:
        print(kernel_table())

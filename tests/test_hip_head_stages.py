"""The diffusion head's fused kernels (csrc/vv_fused.hip: head_pre, head_init, head_sde_proj, adaln_lds, adaln_all, head_boundary,
head_boundary_cfg) and their fallbacks against plain fp64 references, stage by stage - through the C ABI only, no engine, no checkpoint.  Method
and helpers are those of tests/test_hip_mfma_gemm.py and tests/test_hip_conv_block.py.

Every case first asks vv_head_sample_route which stage kernels its arguments take and asserts the route it is named for (the query is host
only, so the route of every case is also asserted on a CPU box with made-up pointers), then reads the workspace regions by vv_head_ws_layout.
Stages are separated by teacher forcing: the reference of a stage starts from what the DEVICE produced for the stage before it, read from the
workspace after the call, so errors do not compound and the bars sit near the arithmetic's floor.
  stage cases   identity steps (alpha_s = 1, sigma_s = 0, cx = 1, cd = 0, order 1: the boundary leaves the state unchanged bit for bit) keep what
                the prologue wrote: c (conditioning rows) against silu(cond_proj cond + temb_i) in fp64 rounded to bf16 ONCE - every element
                within one bf16 step, and the share of elements that differ at all under C_SHARE_CAP; mod[l] / modf against (device c) x adaLN in
                fp64, global / worst 16 x 16 tile / worst row; X0 = [P noise ; noise] (copied part exact), latent_out == noise, final hidden rows
                == Xs[:D] bitwise.  `zr` cases put a z-revealing step (alpha_s = 0, sigma_s = -1, cx = 0, cd = -1) first: the final Xs is step 0's
                z = [P F y ; F y], which depends on the hidden rows h0 the prologue wrote (reference: the head's layers in fp64 from P noise with
                the device's modulations).
  chain cases   calls with n_steps = 5, 6, 7, 8 on the same inputs: four identity steps, then the first 1..4 steps of CHAIN (orders 1, 2 with a
                non-zero previous x0, 2, and a final order-1 step; SDE cases cn != 0 on all but the last).  After the n-step call the workspace
                holds the hidden rows boundary n read, its modf rows and its outputs; the reference computes boundary n in fp64 - RMSNorm,
                modulate, final linear, CFG, DPM-Solver++ update, noisy_images_proj, as modular_vibevoice_diffusion_head.py / dpm_solver.py state
                them, knowing nothing of G - from those rows and the state (x, m) the (n - 1)-step call left ((noise, noise) after the identity
                steps).  Xs, Ms, latent_out: global rel RMS and worst element over the vector's RMS; both h_out rows == Xs[:D] and latent_out ==
                Xs[D:] bitwise.  The identity prefix keeps every call of a chain in one regime: with n_steps = 1..4 the single sampler's
                modulations come from vv_linear on 2, 4, 6, 8 fp32 rows, whose kernels differ in more than summation order, and the state the
                3-step call builds is then not the one the 2-step call left (7e-4 apart at D = 512).
Every call runs twice on separate buffers (bit-identical), with NaN guard rows around latent_out, 0xFF guard bytes around the workspace (whose
interior starts as 0xFF = NaN too), every input and weight held bit-unchanged, every in-range output finite, and the device awaited under
CALL_LIMIT_S.  No vv_tune hook is used.

Bars (BAR) come from the arithmetic, and `test_bars_sit_between_floor_and_faults` (CPU) holds each to: >= 8 x the error of a torch fp32 stand-in
of the stage against the fp64 reference, <= 1/10 of what each fault below, put into the stand-in, costs the figure meant to catch it.
  adaLN     (a) one 32-wide K step dropped in one 16-channel block of one row tile (tile)   (b) a block computed with the weights of the block one
            grid stride later (tile)   (c) a row receiving its clamp neighbour's values (row)   (d) the first block of a matrix not stored where
            it belongs (tile)
  pre       temb of step i + 1 used for step i; cond and uncond rows swapped; one 8-wide K chunk of cond_proj dropped for one output pair: each
            must move some element of c by >= 10 bf16 steps (the check is 1 step); truncation instead of round-to-nearest-even: the share figure
  boundary  one 8-wide slice of G dropped for one state row, Xs or Ms of row g + gstride used for row g (worst element); the order-2 term dropped,
            yc / yu swapped, rs of the other branch, nx of the neighbouring step, cfg of the neighbouring utterance (global)
No (kernel, fault) pair had to be dropped.  Batched cases check every utterance against its own rows; the stand-in given the modulation rows
of utterance b + 1 costs the global figure an order-one error like the other batched faults.

temb of the stage cases is drawn away from zero (temb_away_from_zero says why); one case, pre_ku3_d1536_n20_natural, keeps temb ~ N(0, 1/4) as
real rows are and holds c to |c - ref| <= 2^-8 |ref| + C_ABS instead (c_excess).  The free-running figure: 20-step samples with the production
schedule's coefficients at the 1.5B and the 7B head's D, cond_dim, latent and layer count (7B with a third of its ffn, to keep the CPU reference
short) against ref_sampler, the whole sampler in fp64, under FREE_BAR.

head_sde_proj_kernel<float> is built but reached by no entry point: the batched samplers, the only callers, refuse fp32 weights.  It is listed in
the table below without a case.

Measured on the MI355X, largest value over the class's checks (profiles/head_parity.txt):
  class                          checks   bar (global|tile, worst element|row)  largest / bar  bar / largest
  boundary dpm_proj                  16                        (2e-05, 0.0001)          0.007          136.4
  boundary fused                   1164                        (2e-05, 0.0001)          0.049           20.6
  c fp32                              2                         (1e-05, 5e-05)          0.006          159.3
  c natural                           1                                    1.0          0.003          291.6
  c share                            18                                   0.01          0.020           51.2
  free-running 1p5b                   1                                  0.001          0.000         3478.3
  free-running 7b                     1                                  0.001          0.004          238.6
  mod adaln_all<nst=28,nm=1>         11                         (1e-05, 1e-05)          0.033           29.9
  mod adaln_lds<nst=12>              43                         (1e-05, 1e-05)          0.026           38.4
  mod linear                         12                         (1e-05, 1e-05)          0.096           10.4
  x0                                 53                         (1e-05, 5e-05)          0.034           29.5
  z                                   3                       (5e-05, 0.00025)          0.007          152.5
largest / bar is the largest figure of the class over its own bar (each figure over the bar it is held to).  Nothing comes within 10 x of its
bar; the closest is `mod linear` (10.4 x: fp32 weights and fp32 conditioning rows, fb_f32_n5, where the products are not exact in fp32 as
they are for bf16 x bf16).  Largest share of differing c elements: 2.0e-4 (one bf16 step each).  Free-running 20-step samples: 2.9e-7 (1.5B
head) and 4.2e-6 (7B head) rel RMS against the fp64 whole-sampler reference - the reference rounds c as the device does, so what is left is the
fp32 arithmetic of 20 steps.  Every fault class has a mutated-kernel run that failed its test: profiles/head_parity.txt, section 2.

Kernel -> case ids (generated: `python tests/test_hip_head_stages.py --table`; `test_docstring_table_is_current` keeps it so):
  adaln_all<28,1>            bnd_ku7_full, bnd_b3_cfgsde_d3584, bnd_b2_sde_ku7, bnd_b2_cfgsde_ku7, ... (9 cases)
  adaln_lds<12>              bnd_ku3_full, bnd_b3_d1536, bnd_b8_d1536, bnd_b3_sde, ... (21 cases)
  head_boundary<1,0>         bnd_ku1_full, bnd_ku1_tail72, bnd_d64_lat256, bnd_b2_sde_ku1, ... (8 cases)
  head_boundary<1,1>         bnd_b2_sde_ku1
  head_boundary<2,0>         bnd_ku2_full, bnd_ku2_tail72, bnd_b2_sde_ku2
  head_boundary<2,1>         bnd_b2_sde_ku2
  head_boundary<3,0>         bnd_ku3_full, bnd_ku3_tail72, bnd_f32_d1536, bnd_b3_d1536, ... (21 cases)
  head_boundary<3,1>         bnd_b3_sde, bnd_b2_sde_ku3
  head_boundary<4,0>         bnd_ku4_full, bnd_ku4_tail72, bnd_b2_sde_ku4
  head_boundary<4,1>         bnd_b2_sde_ku4
  head_boundary<5,0>         bnd_ku5_full, bnd_ku5_tail72, bnd_b2_sde_ku5
  head_boundary<5,1>         bnd_b2_sde_ku5
  head_boundary<6,0>         bnd_ku6_full, bnd_ku6_tail72, bnd_b2_sde_ku6
  head_boundary<6,1>         bnd_b2_sde_ku6
  head_boundary<7,0>         bnd_ku7_full, bnd_ku7_tail72, bnd_b2_sde_ku7, pre_ku7_d3584_n5, ... (8 cases)
  head_boundary<7,1>         bnd_b2_sde_ku7
  head_boundary<8,0>         bnd_ku8_full, bnd_ku8_tail72, bnd_b3_d4096, bnd_b8_d4096, ... (5 cases)
  head_boundary<8,1>         bnd_b2_sde_ku8
  head_boundary_cfg<1,0>     bnd_b2_cfgsde_ku1, bnd_b2_cfg_ku1
  head_boundary_cfg<1,1>     bnd_b2_cfgsde_ku1
  head_boundary_cfg<2,0>     bnd_b2_cfgsde_ku2, bnd_b2_cfg_ku2
  head_boundary_cfg<2,1>     bnd_b2_cfgsde_ku2
  head_boundary_cfg<3,0>     bnd_b3_cfg, bnd_b2_cfgsde_ku3, bnd_b2_cfg_ku3
  head_boundary_cfg<3,1>     bnd_b2_cfgsde_ku3
  head_boundary_cfg<4,0>     bnd_b2_cfgsde_ku4, bnd_b2_cfg_ku4
  head_boundary_cfg<4,1>     bnd_b2_cfgsde_ku4
  head_boundary_cfg<5,0>     bnd_b2_cfgsde_ku5, bnd_b2_cfg_ku5
  head_boundary_cfg<5,1>     bnd_b2_cfgsde_ku5
  head_boundary_cfg<6,0>     bnd_b2_cfgsde_ku6, bnd_b2_cfg_ku6
  head_boundary_cfg<6,1>     bnd_b2_cfgsde_ku6
  head_boundary_cfg<7,0>     bnd_b3_cfgsde_d3584, bnd_b2_cfgsde_ku7, bnd_b2_cfg_ku7
  head_boundary_cfg<7,1>     bnd_b3_cfgsde_d3584, bnd_b2_cfgsde_ku7
  head_boundary_cfg<8,0>     bnd_b2_cfgsde_ku8, bnd_b2_cfg_ku8
  head_boundary_cfg<8,1>     bnd_b2_cfgsde_ku8
  head_init<bf16>            bnd_ku1_full, bnd_ku1_tail72, bnd_ku2_full, bnd_ku2_tail72, ... (54 cases)
  head_init<f32>             bnd_f32_d1536, fb_f32_n5
  head_pre<1>                pre_ku1_d1536_n5, fb_d512_modlinear
  head_pre<2>                pre_ku2_d64_n5
  head_pre<3>                pre_ku3_d1536_n20_l4, pre_ku3_d1536_n21, pre_ku3_d1536_n20_l16, zr_ku3_d1536_n5, ... (6 cases)
  head_pre<4>                pre_ku4_d1536_n64
  head_pre<5>                pre_ku5_d1536_n65_lat256
  head_pre<6>                pre_ku6_d64_n128
  head_pre<7>                pre_ku7_d3584_n5, pre_ku7_d3584_n20_l4, zr_ku7_d3584_n5, free_7b
  head_sde_proj<bf16>        bnd_b3_sde, bnd_b3_cfgsde_d3584, bnd_b2_sde_ku1, bnd_b2_cfgsde_ku1, ... (18 cases)
  head_sde_proj<f32>         (no entry point reaches it)
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_mfma_gemm import NAN, _lib, _need_gpu, _rel, _same_bits, bf16_round64, built_kernels, instantiations_of, tile_row_errors

EPS = 1e-5
CALL_LIMIT_S = 20.0
FLOOR_HEADROOM = 8.0
FAULT_MARGIN = 10.0
GUARD = 256

# Chosen from the arithmetic, then checked on the CPU (test_bars_sit_between_floor_and_faults); never from what the device gives.
#   mod       bf16 x bf16 products are exact in fp32, so only the fp32 accumulation of K = 1536 / 3584 terms is left: sqrt(K) 2^-24 = 2..4e-6
#             of the terms' size at the worst, 1e-7..1e-6 as rel RMS.  1e-5 leaves the device another summation order (4 waves x MFMA).  The
#             cheapest fault, a dropped 32-wide step at K = 3584, costs its tile sqrt(32 / 3584) = 9e-2.
#   x0        Xs[:D] = P noise, an fmaf chain over latent <= 256 terms: 1e-6 at the worst -> 1e-5.
#   c_f32     fp32 conditioning rows (cond_proj GEMV + silu in fp32): the dot product's sqrt(K) 2^-24 and expf -> 1e-5.
#   c share   the fp32 prologue rounds to the other bf16 neighbour where its error (1e-6 absolute on c0) crosses a rounding boundary: the share
#             is error / step, 1e-4..1e-3 as the stand-in shows, larger for the small |silu| whose step is small.  Truncation differs from
#             round-to-nearest-even on half of all elements: a tenth of that is 5e-2.  1e-2.
#   boundary  fp32 throughout: the mean of squares, rsqrtf, the modulate, a dot product over D <= 4096 (2^-24 sqrt(D) = 4e-6 of |G||y|) and the
#             solver's few multiplies.  The reference takes P x' where the device carries Xs[:D] along linearly: another 2^-24 per step.
#             Global 2e-5; worst element over the vector's RMS 1e-4 (a 4-sigma element carries 4 x the typical error).  The cheapest fault, an
#             8-wide slice of G dropped at D = 4096, costs its element sqrt(8 / 4096) = 4e-2 of |sigma_s z| >= 1e-2 of the RMS.
#   z         the z-revealing step: the boundary's figure with the layer GEMVs (bf16 weights, fp32 rows, fp32 accumulation over D and ffn)
#             in front: 5e-5.
BAR = {"mod": (1e-5, 1e-5), "x0": (1e-5, 5e-5), "c_f32": (1e-5, 5e-5), "boundary": (2e-5, 1e-4), "z": (5e-5, 2.5e-4)}
C_SHARE_CAP = 1e-2
C_FAULT_STEPS = 10          # a pre fault must move some element of c by at least this many bf16 steps

IDENT = (1.0, 0.0, 1.0, 0.0, 0.0, 1, 0.0)
ZREVEAL = (0.0, -1.0, 0.0, -1.0, 0.0, 1, 0.0)
# (alpha_s, sigma_s, cx, cd, rinv, order, cn): exact in fp32.  Orders 1, 2 (non-zero previous x0), 2, and a final lower-order step
CHAIN = [(0.75, 0.625, 0.875, -0.5, 0.0, 1, 0.0), (0.8125, 0.5625, 0.75, -0.375, 0.75, 2, 0.0), (0.875, 0.4375, 0.6875, -0.4375, 1.25, 2, 0.0),
         (0.9375, 0.3125, 0.5, -0.625, 0.0, 1, 0.0)]
PREFIX = 4
CHAIN_CN = (0.25, 0.1875, 0.125, 0.0)        # SDE: the last step has cn = 0, as sde-dpmsolver++'s has


def coef_rows(n, kind, sde=False):
    if kind == "chain":           # PREFIX identity steps, then the first n - PREFIX steps of the chain
        return [IDENT] * PREFIX + [c[:6] + ((CHAIN_CN[i] if sde else 0.0),) for i, c in enumerate(CHAIN[:n - PREFIX])]
    return [ZREVEAL if (kind == "zr" and i == 0) else IDENT for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """kind: stage (identity steps) | zr (z-revealing step first) | chain.  B = 0: vv_head_sample; B >= 1 with mode batch | sde | cfg."""

    def __init__(self, cid, kind, D, latent, cond_dim, layers, n, route, B=0, mode="single", f32=False, fused=True, ffn=256, scales=None, natural=False):
        self.id, self.kind, self.D, self.latent, self.cond_dim, self.layers, self.n, self.route = cid, kind, D, latent, cond_dim, layers, n, route
        self.B, self.mode, self.f32, self.fused, self.ffn, self.scales = B, mode, f32, fused, ffn, scales
        self.sde = mode in ("sde", "cfgsde", "single_sde")
        self.natural = natural or kind in ("chain", "free")        # temb ~ N(0, 1/4) as drawn; else temb_away_from_zero

    @property
    def Bn(self):
        return max(self.B, 1)


def _pre(ku):
    return f"head_pre<ku={ku}>"


def _bnd(ku, sde=0, cfg=0):
    return f"boundary<ku={ku},sde={sde},cfg={cfg}>"


def _route(pre, mod, step):
    return f"pre={pre} mod={mod} step={step}"


LDS, ALL = "adaln_lds<nst=12>", "adaln_all<nst=28,nm=1>"
FB_BF16 = "linear+add_rows_silu_bf16+head_init<bf16>"


def _cases():
    cs = []

    def add(*a, **kw):
        cs.append(Case(*a, **kw))

    # ---- boundary, every KU (B = 0; n_steps = 5..8 behind the identity prefix: bf16 conditioning rows where D % 32 == 0) ----
    modk = lambda D: {1536: LDS, 3584: ALL}.get(D, "linear")
    for ku in range(1, 9):
        add(f"bnd_ku{ku}_full", "chain", 512 * ku, 64, 64, 1, 8, _route(FB_BF16, modk(512 * ku), _bnd(ku)))
        D = 512 * (ku - 1) + 72            # D % 32 != 0: the conditioning rows stay fp32
        add(f"bnd_ku{ku}_tail72", "chain", D, 24, 64, 1, 8, _route("linear+add_rows_silu+head_init<bf16>", "linear", _bnd(ku)))
    add("bnd_d64_lat256", "chain", 64, 256, 64, 1, 8, _route(FB_BF16, "linear", _bnd(1)))
    add("bnd_f32_d1536", "chain", 1536, 64, 64, 1, 8, _route("linear+add_rows_silu+head_init<f32>", "linear", _bnd(3)), f32=True)
    # ---- boundary, batched: the 256-block cap gives 2 (D = 1536) and 5 (D = 4096) rows per wave ----
    for B in (3, 8):
        add(f"bnd_b{B}_d1536", "chain", 1536, 64, 64, 1, 8, _route(FB_BF16, LDS, _bnd(3)), B=B, mode="batch")
        add(f"bnd_b{B}_d4096", "chain", 4096, 64, 64, 1, 8, _route(FB_BF16, "linear", _bnd(8)), B=B, mode="batch")
    add("bnd_b3_sde", "chain", 1536, 64, 64, 1, 8, _route(FB_BF16 + "+head_sde_proj<bf16>", LDS, _bnd(3, 1)), B=3, mode="sde")
    add("bnd_b3_cfg", "chain", 1536, 64, 64, 1, 8, _route(FB_BF16, LDS, _bnd(3, 0, 1)), B=3, mode="cfg", scales=(0.0, 1.0, 1.75))
    add("bnd_b3_cfgsde_d3584", "chain", 3584, 24, 64, 1, 8, _route(FB_BF16 + "+head_sde_proj<bf16>", ALL, _bnd(7, 1, 1)), B=3, mode="cfgsde", scales=(1.75, 0.0, 1.0))
    # every SDE / per-utterance-guidance instantiation: full D for the SDE forms, a partial last chunk (D = 512 (KU - 1) + 96) for the cfg form
    for ku in range(1, 9):
        mod = {1536: LDS, 3584: ALL}.get(512 * ku, "linear")
        add(f"bnd_b2_sde_ku{ku}", "chain", 512 * ku, 24, 64, 1, 8, _route(FB_BF16 + "+head_sde_proj<bf16>", mod, _bnd(ku, 1)), B=2, mode="sde")
        add(f"bnd_b2_cfgsde_ku{ku}", "chain", 512 * ku, 24, 64, 1, 8, _route(FB_BF16 + "+head_sde_proj<bf16>", mod, _bnd(ku, 1, 1)), B=2, mode="cfgsde", scales=(0.0, 1.75))
        add(f"bnd_b2_cfg_ku{ku}", "chain", 512 * (ku - 1) + 96, 24, 64, 1, 8, _route(FB_BF16, "linear", _bnd(ku, 0, 1)), B=2, mode="cfg", scales=(1.0, 1.75))
    # ---- the three-launch fallback ----
    add("fb_nog_d1536", "chain", 1536, 64, 64, 1, 8, _route("linear+add_rows_silu_bf16", LDS, "dpm_proj"), fused=False)
    add("fb_sde_single", "chain", 1536, 64, 64, 1, 8, _route("linear+add_rows_silu_bf16", LDS, "dpm_proj"), mode="single_sde")
    # ---- head_pre<KU> and the adaLN kernels (identity steps) ----
    add("pre_ku1_d1536_n5", "stage", 1536, 64, 512, 1, 5, _route(_pre(1), LDS, _bnd(3)))
    add("pre_ku2_d64_n5", "stage", 64, 8, 1024, 1, 5, _route(_pre(2), "linear", _bnd(1)))
    add("pre_ku3_d1536_n20_l4", "stage", 1536, 64, 1536, 4, 20, _route(_pre(3), LDS, _bnd(3)))
    add("pre_ku3_d1536_n21", "stage", 1536, 64, 1536, 1, 21, _route(_pre(3), LDS, _bnd(3)))
    add("pre_ku4_d1536_n64", "stage", 1536, 64, 2048, 1, 64, _route(_pre(4), LDS, _bnd(3)))
    add("pre_ku5_d1536_n65_lat256", "stage", 1536, 256, 2560, 1, 65, _route(_pre(5), LDS, _bnd(3)))
    add("pre_ku6_d64_n128", "stage", 64, 8, 3072, 1, 128, _route(_pre(6), "linear", _bnd(1)))
    add("pre_ku7_d3584_n5", "stage", 3584, 64, 3584, 1, 5, _route(_pre(7), ALL, _bnd(7)))
    add("pre_ku7_d3584_n20_l4", "stage", 3584, 64, 3584, 4, 20, _route(_pre(7), ALL, _bnd(7)))
    add("pre_ku3_d1536_n20_l16", "stage", 1536, 64, 1536, 16, 20, _route(_pre(3), LDS, _bnd(3)))
    add("zr_ku3_d1536_n5", "zr", 1536, 64, 1536, 1, 5, _route(_pre(3), LDS, _bnd(3)))
    add("zr_ku7_d3584_n5", "zr", 3584, 64, 3584, 1, 5, _route(_pre(7), ALL, _bnd(7)))
    add("zr_init_bf16_d1536", "zr", 1536, 64, 64, 1, 5, _route(FB_BF16, LDS, _bnd(3)))
    add("pre_ku3_d1536_n20_natural", "stage", 1536, 64, 1536, 1, 20, _route(_pre(3), LDS, _bnd(3)), natural=True)
    # ---- adaLN through the batched samplers: 60 and 320 rows (a last row group of 20 rows / 8 full groups), 48 rows for adaln_all ----
    add("ada_lds_b3_n10_l4", "stage", 1536, 64, 64, 4, 10, _route(FB_BF16, LDS, _bnd(3)), B=3, mode="batch")
    add("ada_lds_b8_n20", "stage", 1536, 64, 64, 1, 20, _route(FB_BF16, LDS, _bnd(3)), B=8, mode="batch")
    add("ada_all_b3_n8", "stage", 3584, 64, 64, 1, 8, _route(FB_BF16, ALL, _bnd(7)), B=3, mode="batch")
    # ---- fallback routes of the prologue ----
    add("fb_n4_f32c", "stage", 1536, 64, 512, 1, 4, _route("linear+add_rows_silu+head_init<bf16>", "linear", _bnd(3)))
    add("fb_n129", "stage", 64, 8, 512, 1, 129, _route(FB_BF16, "linear", _bnd(1)))
    add("fb_d512_modlinear", "stage", 512, 64, 512, 1, 5, _route(_pre(1), "linear", _bnd(1)))
    add("fb_f32_n5", "stage", 1536, 64, 512, 1, 5, _route("linear+add_rows_silu+head_init<f32>", "linear", _bnd(3)), f32=True)
    # ---- free-running 20-step samples at the production heads' D, cond_dim, latent and layer count (7B: a third of its ffn) ----
    add("free_1p5b", "free", 1536, 64, 1536, 4, 20, _route(_pre(3), LDS, _bnd(3)), ffn=4608)
    add("free_7b", "free", 3584, 64, 3584, 4, 20, _route(_pre(7), ALL, _bnd(7)), ffn=3584)
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
HEAD_KERNELS = ["head_pre", "head_init", "head_sde_proj", "head_boundary", "head_boundary_cfg", "adaln_lds", "adaln_all"]
UNREACHED = {"head_sde_proj<f32>"}


def kernels_of(case):
    """the built kernels a case's asserted route names"""
    pre, mod, step = (p.split("=", 1)[1] for p in case.route.split(" "))
    out = set()
    if pre.startswith("head_pre"):
        out.add(f"head_pre<{pre[12:-1]}>")
    for part in pre.split("+"):
        if part.startswith(("head_init", "head_sde_proj")):
            out.add(part)
    if mod != "linear":
        out.add(mod.replace("nst=", "").replace("nm=", ""))
    if step.startswith("boundary"):
        ku, sde, cfg = (int(p.split("=")[1]) for p in step[9:-1].split(","))
        kern = "head_boundary_cfg" if cfg else "head_boundary"
        out.add(f"{kern}<{ku},0>")                        # a chain's last step (cn = 0) and every ODE step
        if sde:
            out.add(f"{kern}<{ku},1>")
    return out


def kernel_table():
    rows = {}
    for c in CASES:
        for k in kernels_of(c):
            rows.setdefault(k, []).append(c.id)
    for k in UNREACHED:
        rows.setdefault(k, [])
    lines = []
    for k in sorted(rows, key=lambda s: (s.split("<")[0], [int(x) if x.isdigit() else x for x in s.split("<")[1][:-1].split(",")])):
        ids = rows[k]
        lines.append(f"  {k:<26} " + (", ".join(ids[:4]) + (f", ... ({len(ids)} cases)" if len(ids) > 4 else "") if ids else "(no entry point reaches it)"))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------------------
# the head: weights drawn here, bf16-rounded once, G built in fp64 as weights.py:_build_head does
# ---------------------------------------------------------------------------------------------------------------
class HeadData:
    def __init__(self, D, latent, cond_dim, layers, ffn, f32=False, fused=True, device="cpu", seed=1):
        self.D, self.latent, self.cond_dim, self.layers, self.ffn, self.f32, self.device = D, latent, cond_dim, layers, ffn, f32, device
        g = torch.Generator(device=device).manual_seed(seed * 7919 + D + 31 * latent + cond_dim)

        def mat(n, k, scale=1.0):
            w = (torch.randn(n, k, generator=g, device=device) * (scale / k ** 0.5)).bfloat16()
            return w.float() if f32 else w

        self.noisy_proj, self.cond_proj = mat(D, latent), mat(D, cond_dim)
        self.final_adaln, self.final_linear = mat(2 * D, D), mat(latent, D)
        self.lay = [dict(norm_w=1 + 0.1 * torch.randn(D, generator=g, device=device), wgate=mat(ffn, D), wup=mat(ffn, D), wdown=mat(D, ffn),
                         adaln=mat(3 * D, D)) for _ in range(layers)]
        P, F = self.noisy_proj.double(), self.final_linear.double()
        self.fused_g = torch.cat([P @ F, F], dim=0).float() if fused else None

    def tensors(self):
        out = [self.noisy_proj, self.cond_proj, self.final_adaln, self.final_linear] + [t for L in self.lay for t in L.values()]
        return out + ([self.fused_g] if self.fused_g is not None else [])

    def desc(self, ptr=lambda t: t.data_ptr()):
        L = _lib()[0]
        layers = (L.HeadLayer * self.layers)()
        for l, d in enumerate(self.lay):
            for k, t in d.items():
                setattr(layers[l], k, ptr(t))
        h = L.Head()
        h.wdt, h.D, h.ffn, h.layers, h.latent, h.cond_dim, h.eps = (0 if self.f32 else 1), self.D, self.ffn, self.layers, self.latent, self.cond_dim, EPS
        h.noisy_proj, h.cond_proj, h.final_adaln, h.final_linear = ptr(self.noisy_proj), ptr(self.cond_proj), ptr(self.final_adaln), ptr(self.final_linear)
        h.layer = C.cast(layers, C.POINTER(L.HeadLayer))
        h.fused_g = ptr(self.fused_g) if self.fused_g is not None else None
        self._keep = layers
        return h


def head_of(case, device):
    return HeadData(case.D, case.latent, case.cond_dim, case.layers, case.ffn, case.f32, case.fused, device)


def inputs_of(case, device):
    g = torch.Generator(device=device).manual_seed(4242 + case.D + case.n)
    r = lambda *s: torch.randn(*s, generator=g, device=device)
    ld_sde = case.n * case.latent + 8
    sde = torch.full((case.Bn, ld_sde), NAN, device=device)
    sde[:, :case.n * case.latent] = r(case.Bn, case.n * case.latent)
    temb = 0.5 * r(case.n, case.D) if case.natural else temb_away_from_zero(r(case.n, case.D), r(case.n, case.D))
    return dict(cond=r(2 * case.Bn, case.cond_dim), noise=r(case.Bn, case.latent), temb=temb, sde=sde, ld_sde=ld_sde)


def temb_away_from_zero(a, b):
    """+-(4 + |N(0, 1)| / 2): with c0 ~ N(0, 1) the sum c0 + temb then stays away from zero.  The one-step check on c is only well posed there: at
    |c0 + temb| < 3e-4 the fp32 error of the dot product (1e-7 absolute) alone is several bf16 steps of silu (2^-8 relative), so natural draws
    (13 such elements among the 61 440 of a 20-step call, and the torch fp32 stand-in 42 steps off on one of them) would fail a correct kernel.
    Both signs occur, so silu is exercised on both branches; the negative branch is the one sensitive to c0 (d ln silu / dv = 0.8 at v = -5)."""
    return torch.sign(a) * (4 + 0.5 * b.abs())


# ---------------------------------------------------------------------------------------------------------------
# references (dt = float64) and, the same text in float32, the stand-ins' prologues
# ---------------------------------------------------------------------------------------------------------------
def ref_c(Wc, cond, temb, dt=torch.float64):
    """silu(cond_proj cond + t_emb(t_i)), row i * rows + r (modular_vibevoice_diffusion_head.py:262-270, :152-156)"""
    c0 = cond.to(dt) @ Wc.to(dt).T
    v = c0[None] + temb.to(dt)[:, None]
    return (v * torch.sigmoid(v)).reshape(-1, Wc.shape[0])


def standin_c(Wc, cond, temb):
    """ref_c in fp32 with cond_proj accumulated as head_pre does it: a lane sums its 8-wide chunks of K, then the 64 lanes are summed - the
    same on every machine, which a library matmul's summation order is not"""
    D, K = Wc.shape
    p = (Wc.float()[:, None, :] * cond.float()[None]).reshape(D, cond.shape[0], K // 512, 64, 8)
    c0 = p.sum((2, 4)).sum(2).T.contiguous()
    v = c0[None] + temb.float()[:, None]
    return (v * torch.sigmoid(v)).reshape(-1, D)


def ref_layers(hd, h, mods, dt=torch.float64):
    """HeadLayer.forward for rows h with their modulation rows mods[l] = [shift | scale | gate]"""
    D = hd.D
    for L, m in zip(hd.lay, mods):
        m = m.to(dt)
        x = h * torch.rsqrt((h * h).mean(1, keepdim=True) + EPS) * L["norm_w"].to(dt).cpu()
        x = x * (1 + m[:, D:2 * D]) + m[:, :D]
        a = x @ L["wgate"].to(dt).cpu().T
        f = (a * torch.sigmoid(a) * (x @ L["wup"].to(dt).cpu().T)) @ L["wdown"].to(dt).cpu().T
        h = h + m[:, 2 * D:] * f
    return h


def ref_boundary(P, F, hrows, modf, x, m, k, cfg, nz=None, dt=torch.float64):
    """FinalLayer + CFG + one DPM-Solver++ update + noisy_images_proj as the model states them (modular_vibevoice_diffusion_head.py:184-188,
    modeling_vibevoice_inference.py:704-707, dpm_solver.py:669-677, 738-764, 993-998).  hrows, modf: [2, .] {cond, uncond}; x, m: [latent]."""
    D = hrows.shape[1]
    P, F, h, modf, x, m = (t.to(dt) for t in (P, F, hrows, modf, x, m))
    a_s, s_s, cx, cd, rinv, order, cn = k
    y = h * torch.rsqrt((h * h).mean(1, keepdim=True) + EPS) * (1 + modf[:, D:]) + modf[:, :D]
    v = y @ F.T
    v = v[1] + cfg * (v[0] - v[1])
    x0 = a_s * x - s_s * v
    xt = cx * x - cd * x0
    if order == 2:
        xt = xt - 0.5 * cd * (rinv * (x0 - m))
    if cn:
        xt = xt + cn * nz.to(dt)
    return dict(Xs=torch.cat([P @ xt, xt]), Ms=torch.cat([P @ x0, x0]), lat=xt)


def standin_boundary(G, hrows, modf, Xs, Ms, k, cfg, nx=None, fault=None, gstride=1024):
    """the kernel's own form in torch fp32: z = G y in 8-wide slices, the solver on the state [P x ; x] element by element"""
    D, N = hrows.shape[1], G.shape[0]
    h, modf, Xs, Ms = hrows.float(), modf.float(), Xs.float().clone(), Ms.float().clone()
    a_s, s_s, cx, cd, rinv, order, cn = k               # exact in fp32; a Python scalar times an fp32 tensor stays fp32
    rs = torch.rsqrt((h * h).mean(1, keepdim=True) + EPS)
    if fault == "rs":
        rs = rs.flip(0)
    y = h * rs * (1 + modf[:, D:]) + modf[:, :D]
    yc, yu = (y[1], y[0]) if fault == "swap" else (y[0], y[1])
    yy = yu + cfg * (yc - yu)
    part = (G.reshape(N, D // 8, 8) * yy.reshape(D // 8, 8)).sum(2)
    if fault == "gslice":
        part[N // 3, (D // 8) // 2] = 0
    z = part.sum(1)
    g = N // 5
    if fault == "nbr_x":
        Xs[g] = Xs[(g + gstride) % N]
    if fault == "nbr_m":
        Ms[g] = Ms[(g + gstride) % N]
    x0 = a_s * Xs - s_s * z
    xt = cx * Xs - cd * x0
    if order == 2 and fault != "order2":
        xt = xt - 0.5 * cd * (rinv * (x0 - Ms))
    if cn:
        xt = xt + cn * nx.float()
    return dict(Xs=xt, Ms=x0, lat=xt[D:])


def vec_errors(got, ref):
    """(global rel RMS, worst element over the vector's RMS)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    rms = np.sqrt(np.mean(ref ** 2)) + 1e-300
    return float(np.sqrt(np.mean((got - ref) ** 2)) / rms), float(np.abs(got - ref).max() / rms)


def bf16_steps(a, b):
    """distance in bf16 steps between two bf16 tensors, element by element"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


def c_figures(c_bf16, ref64):
    """(largest distance in bf16 steps, share of elements that differ) of bf16 rows against the correctly rounded fp64 value"""
    want = bf16_round64(ref64).to(torch.bfloat16)
    d = bf16_steps(c_bf16.cpu(), want)
    return int(d.max()), float((d != 0).double().mean())


C_ABS = 1.5e-5


def c_excess(c_bf16, ref64):
    """largest (|c - ref| - 2^-8 |ref|) / C_ABS: a correctly rounded bf16 value is within 2^-9 |ref| of ref and one step more is allowed as for
    the other cases; what is left must be under C_ABS = 1.5e-5, the fp32 error of the pre-activation: a K <= 3584 dot product of O(1) sums accumulates
    sqrt(K) 2^-24 = 3.6e-6 rms in a sequential order, 4 sigma of that over the 61 440 elements of a call is 1.4e-5, and |silu'| <= 1.1"""
    c, ref = c_bf16.double().cpu(), ref64
    return float(((c - ref).abs() - 2.0 ** -8 * ref.abs()).max() / C_ABS)


def ref_sampler(hd, cond, noise, temb, coefs, cfg, dt=torch.float64):
    """sample_speech_tokens for one utterance as the model states it, in dt on the CPU; the one rounding is c to bf16 (the device's design).
    dt = float32 is the stand-in of the free-running figure."""
    cpu = lambda t: t.to("cpu").to(dt)
    D = hd.D
    c = ref_c(cpu(hd.cond_proj), cond.cpu(), temb.cpu(), dt)
    c = bf16_round64(c) if dt == torch.float64 else c.bfloat16().to(dt)
    lay = [{k: cpu(v) for k, v in L.items()} for L in hd.lay]
    mods = [c @ L["adaln"].T for L in lay]
    modf = c @ cpu(hd.final_adaln).T
    P, F = cpu(hd.noisy_proj), cpu(hd.final_linear)
    x, m = noise.cpu().to(dt), torch.zeros(hd.latent, dtype=dt)
    for i, k in enumerate(coefs):
        h = (P @ x).expand(2, D).clone()
        for L, md in zip(lay, mods):
            mr = md[2 * i:2 * i + 2]
            xn = h * torch.rsqrt((h * h).mean(1, keepdim=True) + EPS) * L["norm_w"]
            xn = xn * (1 + mr[:, D:2 * D]) + mr[:, :D]
            a = xn @ L["wgate"].T
            h = h + mr[:, 2 * D:] * ((a * torch.sigmoid(a) * (xn @ L["wup"].T)) @ L["wdown"].T)
        out = ref_boundary(P, F, h, modf[2 * i:2 * i + 2], x, m, k, cfg, dt=dt)
        x, m = out["lat"], out["Ms"][D:]
    return x


def production_coefs(n=20):
    from vibevoice_rocm_amd.schedule import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler()
    sch.set_timesteps(n)
    f = lambda v: float(np.float32(v))
    return [(f(c["alpha_s"]), f(c["sigma_s"]), f(c["cx"]), f(c["cd"]), f(c["rinv"]), c["order"], f(c["cn"])) for c in sch.coefs]


def standin_adaln(c_bf16, W, fault=None, grid_cols=4096):
    """fp32, accumulated in the kernel's 32-wide K steps; c [rows, K] bf16, W [n, K] bf16 (all matrices of the walk stacked)"""
    c, W = c_bf16.float(), W.float()
    acc = torch.zeros(c.shape[0], W.shape[0])
    for s in range(c.shape[1] // 32):
        p = c[:, 32 * s:32 * s + 32] @ W[:, 32 * s:32 * s + 32].T
        if fault == "a" and s == 7:
            p[:16, 16:32] = 0
        acc = acc + p
    if fault == "b":
        acc[:, 32:48] = acc[:, 32 + grid_cols:48 + grid_cols].clone()
    if fault == "c":
        acc[c.shape[0] - 1] = acc[c.shape[0] - 2]
    if fault == "d":
        acc[:, -W.shape[0] // 5 * 2:][:, :16] = 0
    return acc


# ---------------------------------------------------------------------------------------------------------------
# CPU: the bars, the table, the built kernels, the queries' argument errors and every case's route
# ---------------------------------------------------------------------------------------------------------------
def test_identity_step_keeps_the_state_bit_for_bit():
    g = torch.Generator().manual_seed(3)
    D, lat = 64, 24
    G = torch.randn(D + lat, D, generator=g)
    Xs, Ms = torch.randn(D + lat, generator=g), torch.randn(D + lat, generator=g)
    out = standin_boundary(G, torch.randn(2, D, generator=g), torch.randn(2, 2 * D, generator=g), Xs, Ms, IDENT, 1.3)
    assert _same_bits(out["Xs"], Xs) and _same_bits(out["Ms"], Xs)
    z = standin_boundary(G, torch.ones(2, D), torch.zeros(2, 2 * D), Xs, Ms, ZREVEAL, 1.0)
    y = torch.ones(D) * torch.rsqrt(torch.tensor(1.0 + EPS))
    assert torch.allclose(z["Xs"], G @ y, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("D", [1536, 3584])
def test_bars_sit_between_floor_and_faults_adaln(D):
    g = torch.Generator().manual_seed(D)
    rows = 10
    c = (0.5 * torch.randn(rows, D, generator=g)).bfloat16()
    W = (torch.randn(5 * D, D, generator=g) / D ** 0.5).bfloat16()
    ref = c.double() @ W.double().T
    base = standin_adaln(c, W)
    t, _, r, _ = tile_row_errors(base, ref, 16, 16)
    floor = (max(_rel(base, ref), t), r)
    assert BAR["mod"][0] >= FLOOR_HEADROOM * floor[0] and BAR["mod"][1] >= FLOOR_HEADROOM * floor[1], floor
    for fault, fig in (("a", 0), ("b", 0), ("c", 1), ("d", 0)):
        t, _, r, _ = tile_row_errors(standin_adaln(c, W, fault), ref, 16, 16)
        assert BAR["mod"][fig] <= (t, r)[fig] / FAULT_MARGIN, (fault, t, r)


@pytest.mark.parametrize("ku,D,n", [(1, 64, 5), (3, 1536, 20), (7, 3584, 5)])
def test_bars_sit_between_floor_and_faults_pre(ku, D, n):
    g = torch.Generator().manual_seed(ku)
    K = 512 * ku
    Wc = (torch.randn(D, K, generator=g) / K ** 0.5).bfloat16()
    cond, temb = torch.randn(2, K, generator=g), temb_away_from_zero(torch.randn(n, D, generator=g), torch.randn(n, D, generator=g))
    ref = ref_c(Wc, cond, temb)
    s32 = standin_c(Wc, cond, temb)
    steps, share = c_figures(s32.bfloat16(), ref)
    trunc = (s32.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    _, share_trunc = c_figures(trunc, ref)
    assert steps <= 1 and C_SHARE_CAP >= FLOOR_HEADROOM * share and C_SHARE_CAP <= share_trunc / FAULT_MARGIN, (steps, share, share_trunc)
    f_ref, f_std = vec_errors(s32, ref)
    assert BAR["c_f32"][0] >= FLOOR_HEADROOM * f_ref and BAR["c_f32"][1] >= FLOOR_HEADROOM * f_std, (f_ref, f_std)
    nat = 0.5 * torch.randn(n, D, generator=g)              # natural temb: the relative criterion, floor and faults
    rn, sn = ref_c(Wc, cond, nat), standin_c(Wc, cond, nat)
    assert float((sn.double() - rn).abs().max()) <= C_ABS / FLOOR_HEADROOM and c_excess(sn.bfloat16(), rn) < 1.0 / FLOOR_HEADROOM
    assert c_excess(standin_c(Wc, cond.flip(0), nat).bfloat16(), rn) >= FAULT_MARGIN
    assert c_excess(standin_c(Wc, cond, nat.roll(-1, 0)).bfloat16(), rn) >= FAULT_MARGIN
    Wd = Wc.clone()
    Wd[2:4, 8:16] = 0                                       # one 8-wide K chunk dropped for the output pair (2, 3)
    faults = {"temb": standin_c(Wc, cond, temb.roll(-1, 0)), "swap": standin_c(Wc, cond.flip(0), temb), "chunk": standin_c(Wd, cond, temb)}
    assert c_excess(standin_c(Wd, cond, nat).bfloat16(), rn) >= FAULT_MARGIN
    for name, f in faults.items():
        assert c_figures(f.bfloat16(), ref)[0] >= C_FAULT_STEPS, name
        assert BAR["c_f32"][1] <= vec_errors(f, ref)[1] / FAULT_MARGIN, name


@pytest.mark.parametrize("D,lat", [(4096, 64), (72, 24), (1536, 256)])
def test_bars_sit_between_floor_and_faults_boundary(D, lat):
    g = torch.Generator().manual_seed(D + lat)
    r = lambda *s: torch.randn(*s, generator=g)
    P, F = (r(D, lat) / lat ** 0.5).bfloat16(), (r(lat, D) / D ** 0.5).bfloat16()
    G = torch.cat([P.double() @ F.double(), F.double()]).float()
    h, modf, x, m, nz, nz2 = r(2, D), 0.3 * r(2, 2 * D), r(lat), r(lat), r(lat), r(lat)
    st = lambda v: torch.cat([P.float() @ v, v])
    k = CHAIN[1][:6] + (0.25,)
    fl = vec_errors(P.float() @ x, P.double() @ x.double())
    assert BAR["x0"][0] >= FLOOR_HEADROOM * fl[0] and BAR["x0"][1] >= FLOOR_HEADROOM * fl[1], fl
    ref = ref_boundary(P, F, h, modf, x, m, k, 1.75, nz)
    base = standin_boundary(G, h, modf, st(x), st(m), k, 1.75, st(nz))
    for q in ("Xs", "Ms"):
        fl = vec_errors(base[q], ref[q])
        assert BAR["boundary"][0] >= FLOOR_HEADROOM * fl[0] and BAR["boundary"][1] >= FLOOR_HEADROOM * fl[1], (q, fl)
    cost = lambda out, q, fig: vec_errors(out[q], ref[q])[fig]
    sb = lambda **kw: standin_boundary(G, h, modf, st(x), st(m), k, 1.75, st(nz), **kw)
    assert BAR["boundary"][1] <= cost(sb(fault="gslice"), "Ms", 1) / FAULT_MARGIN
    assert BAR["boundary"][1] <= cost(sb(fault="gslice"), "Xs", 1) / FAULT_MARGIN
    assert BAR["boundary"][1] <= cost(sb(fault="nbr_x", gstride=min(1024, D // 2)), "Xs", 1) / FAULT_MARGIN
    assert BAR["boundary"][1] <= cost(sb(fault="nbr_m", gstride=min(1024, D // 2)), "Xs", 1) / FAULT_MARGIN
    for fault in ("order2", "swap", "rs"):
        assert BAR["boundary"][0] <= cost(sb(fault=fault), "Xs", 0) / FAULT_MARGIN, fault
    assert BAR["boundary"][0] <= cost(standin_boundary(G, h, modf, st(x), st(m), k, 1.75, st(nz2)), "Xs", 0) / FAULT_MARGIN       # nx of the neighbouring step / utterance: its own draw
    # batched: utterance b computed from the modulation rows of utterance b + 1 (their own draw, as 2 (b + 1), 2 (b + 1) + 1 of a call hold)
    modf_b1 = 0.3 * r(2, 2 * D)
    assert BAR["boundary"][0] <= cost(standin_boundary(G, h, modf_b1, st(x), st(m), k, 1.75, st(nz)), "Xs", 0) / FAULT_MARGIN
    assert BAR["boundary"][0] <= cost(standin_boundary(G, h, modf_b1, st(x), st(m), k, 1.75, st(nz)), "Ms", 0) / FAULT_MARGIN
    assert BAR["boundary"][0] <= cost(standin_boundary(G, h, modf, st(x), st(m), k, 1.0, st(nz)), "Xs", 0) / FAULT_MARGIN        # cfg of a neighbour
    # the z-revealing step sees the same faults at sigma_s = -1; its bar is the boundary's with the layers in front
    assert BAR["z"][0] >= BAR["boundary"][0] and BAR["z"][0] <= cost(sb(fault="swap"), "Xs", 0) / FAULT_MARGIN


def test_docstring_table_is_current():
    assert kernel_table() in __doc__
    named = {k.split("<")[0] for c in CASES for k in kernels_of(c)}
    assert named == set(HEAD_KERNELS), named ^ set(HEAD_KERNELS)


NAMES = {"head_pre_kernel": lambda ku: f"head_pre<{ku}>", "head_init_kernel": lambda t: f"head_init<{t}>",
         "head_sde_proj_kernel": lambda t: f"head_sde_proj<{t}>", "head_boundary_kernel": lambda ku, s: f"head_boundary<{ku},{s}>",
         "head_boundary_cfg_kernel": lambda ku, s: f"head_boundary_cfg<{ku},{s}>", "adaln_lds_kernel": lambda n: f"adaln_lds<{n}>",
         "adaln_all_kernel": lambda n, m: f"adaln_all<{n},{m}>"}


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """vv_fused.hip's code object holds the head kernels the cases' routes name, those listed as unreached, and - of the KU templates - the
    instantiations no listed shape needs are named here: none"""
    got = instantiations_of(built_kernels("vv_fused.hip", tmp_path), NAMES)
    want = {k for c in CASES for k in kernels_of(c)} | UNREACHED
    assert got == want, sorted(got ^ want)


_FAKE = {"cond": 0x10000000, "temb": 0x20000000, "ws": 0x30000000, "cfg": 0x40000000, "w": 0x50000000}


def route_of(case, h, n, cond, temb, ws, cfg_rows, coefs):
    L, l = _lib()[:2]
    arr = (L.DpmCoef * n)(*[L.DpmCoef(*c) for c in coefs])
    name = C.create_string_buffer(160)
    B = case.B if case.mode != "single_sde" else 0
    rc = l.vv_head_sample_route(C.byref(h), cond, case.cond_dim, temb, arr, n, B, int(case.sde), cfg_rows if case.mode in ("cfg", "cfgsde") else None,
                                ws, name, 160)
    assert rc == 0, l.vv_last_error().decode()
    return name.value.decode()


def layout_of(h, n, B, sde):
    l = _lib()[1]
    off = (C.c_int64 * 40)()
    k = l.vv_head_ws_layout(C.byref(h), n, B, int(sde), off, 40)
    assert k > 0, l.vv_last_error().decode()
    names = ["c0", "c"] + [f"mod{i}" for i in range(h.layers)] + ["modf", "h0", "h1", "act", "Xs", "Ms", "NX"] + \
        (["v", "xb0", "xb1", "mb0", "mb1"] if B == 0 else []) + ["end"]
    assert k == len(names)
    return dict(zip(names, list(off)[:k]))


def ws_bytes_of(h, n, B, sde):
    l = _lib()[1]
    if B == 0:
        return l.vv_head_ws_bytes(C.byref(h), n)
    return (l.vv_head_ws_bytes_batch_sde if sde else l.vv_head_ws_bytes_batch)(C.byref(h), n, B)


class _Fake:       # a tensor stand-in for HeadData.desc on a CPU box: aligned made-up addresses
    def __init__(self):
        self.next = _FAKE["w"]

    def __call__(self, t):
        self.next += 1 << 28
        return self.next


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_and_layout_of_every_case_on_the_host(cid):
    case = CASES[CASE_IDS.index(cid)]
    hd = HeadData(8, 8, 8, case.layers, 8, case.f32, case.fused)          # tiny tensors: only the descriptor's numbers and addresses count
    h = hd.desc(_Fake())
    h.D, h.latent, h.cond_dim, h.ffn = case.D, case.latent, case.cond_dim, case.ffn
    if not case.fused:
        h.fused_g = None
    nmax = case.n
    for n in (range(PREFIX + 1, nmax + 1) if case.kind == "chain" else (nmax,)):
        coefs = coef_rows(n, case.kind, case.sde)
        assert route_of(case, h, n, _FAKE["cond"], _FAKE["temb"], _FAKE["ws"], _FAKE["cfg"], coefs) == case.route       # a chain's shorter calls take the same route
    B = case.B if case.mode != "single_sde" else 0
    lay = layout_of(h, nmax, B, case.sde and B > 0)
    assert lay["end"] == ws_bytes_of(h, nmax, B, case.sde and B > 0)
    offs = [v for k, v in lay.items() if v >= 0 and k != "end"]
    assert all(o % 256 == 0 for o in offs) and len(set(offs)) == len(offs) and max(offs) < lay["end"]
    assert (lay["NX"] >= 0) == (case.sde and B > 0)


def test_queries_refuse_what_the_samplers_refuse():
    L, l = _lib()[:2]
    hd = HeadData(64, 8, 64, 1, 64)
    h = hd.desc(_Fake())
    name = C.create_string_buffer(160)
    ident = (L.DpmCoef * 5)(*[L.DpmCoef(*IDENT) for _ in range(5)])
    sdec = (L.DpmCoef * 5)(*[L.DpmCoef(*(IDENT[:6] + (0.5,))) for _ in range(5)])
    q = lambda hh, cond, temb, coef, n, B, sde, cfg, ws, nm=name, cap=160: l.vv_head_sample_route(hh, cond, 64, temb, coef, n, B, sde, cfg, ws, nm, cap)
    E_ARG, E_UNS = q(C.byref(h), 1 << 20, 1 << 21, ident, 5, 0, 0, None, 1 << 22, None, 0), None
    assert E_ARG < 0
    assert q(None, 1 << 20, 1 << 21, ident, 5, 0, 0, None, 1 << 22) == E_ARG
    assert q(C.byref(h), None, 1 << 21, ident, 5, 0, 0, None, 1 << 22) == E_ARG and b"vv_head_sample" in l.vv_last_error()
    assert q(C.byref(h), 1 << 20, 1 << 21, ident, 0, 0, 0, None, 1 << 22) == E_ARG
    assert q(C.byref(h), 1 << 20, 1 << 21, ident, 5, 9, 0, None, 1 << 22) == E_ARG and b"vv_head_sample_batch" in l.vv_last_error()
    assert q(C.byref(h), 1 << 20, 1 << 21, ident, 5, -1, 0, None, 1 << 22) == E_ARG
    assert q(C.byref(h), 1 << 20, 1 << 21, ident, 5, 0, 0, 1 << 23, 1 << 22) == E_ARG
    E_UNS = q(C.byref(h), 1 << 20, 1 << 21, sdec, 5, 2, 0, None, 1 << 22)          # SDE coefficients at vv_head_sample_batch
    assert E_UNS < 0 and E_UNS != E_ARG and b"vv_head_sample_batch_sde" in l.vv_last_error()
    assert q(C.byref(h), 1 << 20, 1 << 21, sdec, 5, 2, 0, 1 << 23, 1 << 22) == E_ARG          # _cfg without the variance noise its steps need
    assert q(C.byref(h), 1 << 20, 1 << 21, sdec, 5, 2, 1, None, 1 << 22) == 0 and b"sde=1" in name.value
    hf = HeadData(64, 8, 64, 1, 64, f32=True).desc(_Fake())
    assert q(C.byref(hf), 1 << 20, 1 << 21, ident, 5, 2, 0, None, 1 << 22) == E_UNS           # fp32 weights, batched
    assert q(C.byref(hf), 1 << 20, 1 << 21, ident, 5, 0, 0, None, 1 << 22) == 0 and name.value.decode() == _route("linear+add_rows_silu+head_init<f32>", "linear", _bnd(1))
    # alignment decides: a workspace at an odd 4-byte address keeps the conditioning rows in fp32; an unaligned cond keeps head_pre away
    hp = HeadData(64, 8, 512, 1, 64).desc(_Fake())
    q2 = lambda cond, ws: (l.vv_head_sample_route(C.byref(hp), cond, 512, 1 << 21, ident, 5, 0, 0, None, ws, name, 160), name.value.decode())[1]
    assert q2(1 << 20, 1 << 22) == _route(_pre(1), "linear", _bnd(1))
    assert q2((1 << 20) + 4, 1 << 22) == _route(FB_BF16, "linear", _bnd(1))
    assert q2(1 << 20, (1 << 22) + 4) == _route("linear+add_rows_silu+head_init<bf16>", "linear", _bnd(1))
    off = (C.c_int64 * 40)()
    w = lambda hh, n, B, sde, o=off, cap=40: l.vv_head_ws_layout(hh, n, B, sde, o, cap)
    assert w(None, 5, 0, 0) == E_ARG and w(C.byref(h), 0, 0, 0) == E_ARG and w(C.byref(h), 5, 9, 0) == E_ARG and w(C.byref(h), 5, 0, 1) == E_ARG
    assert w(C.byref(h), 5, 0, 0, None) == E_ARG and w(C.byref(h), 5, 0, 0, off, 15) == E_ARG and w(C.byref(h), 5, 0, 0, off, 16) == 16
    assert w(C.byref(h), 5, 2, 0, off, 11) == 11 and off[9] == -1 and w(C.byref(h), 5, 2, 1, off, 11) == 11 and off[9] > 0
    assert l.vv_abi_version() == 6


# ---------------------------------------------------------------------------------------------------------------
# GPU: one sampler call with guards, twice
# ---------------------------------------------------------------------------------------------------------------
def _wait(what):
    ev = torch.cuda.Event()
    ev.record()
    end = time.monotonic() + CALL_LIMIT_S
    while not ev.query():
        assert time.monotonic() < end, f"{what}: not finished after {CALL_LIMIT_S} s"
        time.sleep(0)


_MEASURED = {}


def _note(klass, bar, *figs):
    m = _MEASURED.setdefault(klass, [bar, 0, 0.0])
    m[1] += 1
    m[2] = max(m[2], max(f / b for f, b in zip(figs, bar if isinstance(bar, tuple) else (bar,) * len(figs))))


def call_sampler(case, hd, h, inp, n, coefs, cfg=1.75):
    """one call on fresh buffers: (regions {name: fp32 / bf16 tensor on the CPU}, latent_out [Bn, latent])"""
    L, l = _lib()[:2]
    Bn, lat, D = case.Bn, case.latent, case.D
    B = case.B if case.mode != "single_sde" else 0
    sde_ws = case.sde and B > 0
    size = ws_bytes_of(h, n, B, sde_ws)
    buf = torch.full((GUARD + size + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = buf.data_ptr() + GUARD
    ld_lat = lat + 4
    out = torch.full((Bn + 2, ld_lat), NAN, device="cuda")
    cfg_rows = torch.tensor(case.scales, device="cuda") if case.scales else None
    arr = (L.DpmCoef * n)(*[L.DpmCoef(*c) for c in coefs])
    ins = [inp["cond"], inp["noise"], inp["temb"], inp["sde"]] + ([cfg_rows] if cfg_rows is not None else []) + hd.tensors()
    before = [t.clone() for t in ins]
    assert route_of(case, h, n, inp["cond"].data_ptr(), inp["temb"].data_ptr(), ws, cfg_rows.data_ptr() if cfg_rows is not None else None, coefs) == case.route
    a = (C.byref(h), inp["cond"].data_ptr(), case.cond_dim, inp["noise"].data_ptr())
    optr = out[1:].data_ptr()
    if B == 0:
        rc = l.vv_head_sample(*a, inp["temb"].data_ptr(), arr, n, cfg, optr, ws, inp["sde"].data_ptr() if case.sde else None, None)
    elif case.mode == "batch":
        rc = l.vv_head_sample_batch(*a, lat, inp["temb"].data_ptr(), arr, n, 1.75, optr, ld_lat, B, ws, None)
    elif case.mode == "sde":
        rc = l.vv_head_sample_batch_sde(*a, lat, inp["temb"].data_ptr(), arr, n, 1.75, optr, ld_lat, B, ws, inp["sde"].data_ptr(), inp["ld_sde"], None)
    else:
        rc = l.vv_head_sample_batch_cfg(*a, lat, inp["temb"].data_ptr(), arr, n, cfg_rows.data_ptr(), optr, ld_lat, B, ws,
                                        inp["sde"].data_ptr() if case.sde else None, inp["ld_sde"] if case.sde else 0, None)
    L.check(rc, case.id)
    _wait(case.id)
    assert all(_same_bits(x, y) for x, y in zip(ins, before)), "an input or a weight changed"
    assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + size:] == 0xFF).all()), "workspace guard bytes"
    o = out.cpu()
    assert bool(torch.isnan(o[0]).all()) and bool(torch.isnan(o[-1]).all()) and bool(torch.isnan(o[:, lat:]).all()), "latent_out guards"
    assert bool(torch.isfinite(o[1:-1, :lat]).all())
    lay = layout_of(h, n, B, sde_ws)
    assert lay["end"] == size
    raw = buf[GUARD:GUARD + size].cpu()

    def region(name, shape, dtype=torch.float32):
        nb = int(np.prod(shape)) * (2 if dtype == torch.bfloat16 else 4)
        return raw[lay[name]:lay[name] + nb].view(dtype).reshape(shape).clone()
    return region, o[1:-1, :lat].clone(), lay


def _teacher_chain(case, hd, h, inp):
    P, F = hd.noisy_proj.double().cpu(), hd.final_linear.double().cpu()
    D, lat, Bn, R2 = case.D, case.latent, case.Bn, 2 * case.Bn
    N = D + lat
    noise = inp["noise"].cpu().double()
    prev = None
    fused = "boundary" in case.route
    for k in range(PREFIX + 1, case.n + 1):
        coefs = coef_rows(k, "chain", case.sde)
        r1, lat1, lay = call_sampler(case, hd, h, inp, k, coefs)
        r2, lat2, _ = call_sampler(case, hd, h, inp, k, coefs)
        modf = r1("modf", (R2 * k, 2 * D))
        hin = r1("h1" if (fused and (k - 1) & 1) else "h0", (R2, D))
        assert _same_bits(lat1, lat2) and _same_bits(modf, r2("modf", (R2 * k, 2 * D)))
        if fused:
            Xs, Ms, hout = r1("Xs", (Bn, N)), r1("Ms", (Bn, N)), r1("h1" if k & 1 else "h0", (R2, D))
            assert _same_bits(Xs, r2("Xs", (Bn, N))) and _same_bits(Ms, r2("Ms", (Bn, N)))
            assert bool(torch.isfinite(Xs).all()) and bool(torch.isfinite(Ms).all())
            for b in range(Bn):
                assert _same_bits(hout[2 * b], Xs[b, :D]) and _same_bits(hout[2 * b + 1], Xs[b, :D]), "h_out rows != Xs[:D]"
                assert _same_bits(lat1[b], Xs[b, D:]), "latent_out != Xs[D:]"
            state = (Xs[:, D:].double(), Ms[:, D:].double())
        else:
            Ms = r1("mb1" if k & 1 else "mb0", (1, lat))
            assert _same_bits(Ms, r2("mb1" if k & 1 else "mb0", (1, lat)))
            state = (lat1.double(), Ms.double())
        for b in range(Bn):
            x, m = (noise[b], noise[b]) if prev is None else (prev[0][b], prev[1][b])       # after identity steps M = x0 = X
            cfg = case.scales[b] if case.scales else 1.75
            nz = inp["sde"][b, (k - 1) * lat:k * lat].cpu() if case.sde else None
            ref = ref_boundary(P, F, hin[2 * b:2 * b + 2], modf[R2 * (k - 1) + 2 * b:R2 * (k - 1) + 2 * b + 2], x, m, coefs[k - 1], cfg, nz)
            got = dict(Xs=Xs[b], Ms=Ms[b], lat=lat1[b]) if fused else dict(lat=lat1[b], Ms=Ms[0])
            for q, v in got.items():
                rq = ref[q] if (fused or q == "lat") else ref["Ms"][D:]
                e = vec_errors(v, rq)
                print(f"{case.id} k={k} b={b} {q}: global {e[0]:.2e} worst element {e[1]:.2e}")
                _note("boundary " + ("fused" if fused else "dpm_proj"), BAR["boundary"], *e)
                assert e[0] < BAR["boundary"][0] and e[1] < BAR["boundary"][1], (case.id, k, b, q, e)
        prev = state


def _stage(case, hd, h, inp):
    D, lat, Bn, R2, n = case.D, case.latent, case.Bn, 2 * case.Bn, case.n
    N, rows = D + lat, 2 * case.Bn * case.n
    coefs = coef_rows(n, case.kind)
    r1, lat1, lay = call_sampler(case, hd, h, inp, n, coefs)
    r2, lat2, _ = call_sampler(case, hd, h, inp, n, coefs)
    bf = "_bf16" in case.route or "head_pre" in case.route
    c = r1("c", (rows, D), torch.bfloat16 if bf else torch.float32)
    mods = [r1(f"mod{l}", (rows, 3 * D)) for l in range(case.layers)]
    modf, Xs, Ms = r1("modf", (rows, 2 * D)), r1("Xs", (Bn, N)), r1("Ms", (Bn, N))
    hfin = r1("h1" if n & 1 else "h0", (R2, D))
    assert _same_bits(lat1, lat2) and _same_bits(c, r2("c", (rows, D), c.dtype)) and _same_bits(modf, r2("modf", (rows, 2 * D))) and _same_bits(Xs, r2("Xs", (Bn, N)))
    assert all(_same_bits(m, r2(f"mod{l}", (rows, 3 * D))) for l, m in enumerate(mods))
    # ---- c ----
    cref = ref_c(hd.cond_proj.cpu(), inp["cond"].cpu(), inp["temb"].cpu())
    if bf:
        if case.natural:             # natural temb: c0 + temb crosses zero, where a bf16 step of silu is smaller than the dot product's fp32 error
            ex = c_excess(c, cref)
            print(f"{case.id} c (natural temb): largest (|c - ref| - 2^-8 |ref|) / C_ABS = {ex:.3f}")
            _note("c natural", 1.0, ex)
            assert ex < 1.0, (case.id, ex)
        else:
            steps, share = c_figures(c, cref)
            print(f"{case.id} c: largest distance {steps} bf16 steps, share differing {share:.2e}")
            _note("c share", C_SHARE_CAP, share)
            assert steps <= 1 and share < C_SHARE_CAP, (case.id, steps, share)
    else:
        e = vec_errors(c, cref)
        print(f"{case.id} c (fp32): global {e[0]:.2e} worst element {e[1]:.2e}")
        _note("c fp32", BAR["c_f32"], *e)
        assert e[0] < BAR["c_f32"][0] and e[1] < BAR["c_f32"][1], (case.id, e)
    # ---- mod[l], modf from the device's c ----
    c64 = c.double()
    for l, (got, W) in enumerate(zip(mods + [modf], [L["adaln"] for L in hd.lay] + [hd.final_adaln])):
        ref = c64 @ W.cpu().double().T
        assert bool(torch.isfinite(got).all())
        t, ti, r, ri = tile_row_errors(got, ref, 16, 16)
        gl = _rel(got, ref)
        print(f"{case.id} mod[{l}]: global {gl:.2e} tile {t:.2e} {ti} row {r:.2e} ({ri})")
        _note("mod " + case.route.split(" ")[1][4:], BAR["mod"], max(gl, t), r)
        assert max(gl, t) < BAR["mod"][0] and r < BAR["mod"][1], (case.id, l, gl, t, ti, r, ri)
    # ---- the state ----
    P, noise = hd.noisy_proj.double().cpu(), inp["noise"].cpu()
    for b in range(Bn):
        assert _same_bits(lat1[b], Xs[b, D:]) and _same_bits(hfin[2 * b], Xs[b, :D]) and _same_bits(hfin[2 * b + 1], Xs[b, :D])
        h0 = P @ noise[b].double()
        if case.kind == "stage":
            assert _same_bits(Xs[b, D:], noise[b]) and _same_bits(lat1[b], noise[b]), "identity steps: the copied part of X0"
            e = vec_errors(Xs[b, :D], h0)
            _note("x0", BAR["x0"], *e)
            assert e[0] < BAR["x0"][0] and e[1] < BAR["x0"][1], (case.id, b, e)
        else:                      # step 0 revealed z: the layers in fp64 from h0 = P noise with the device's modulation rows of step 0
            rows0 = slice(2 * b, 2 * b + 2)
            hl = ref_layers(hd, torch.stack([h0, h0]), [m[rows0] for m in mods])
            ref = ref_boundary(P, hd.final_linear.double().cpu(), hl, modf[rows0], torch.zeros(lat), torch.zeros(lat), ZREVEAL, 1.75)
            e = vec_errors(Xs[b], ref["Xs"])
            print(f"{case.id} z b={b}: global {e[0]:.2e} worst element {e[1]:.2e}")
            _note("z", BAR["z"], *e)
            assert e[0] < BAR["z"][0] and e[1] < BAR["z"][1], (case.id, b, e)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES if c.kind != "free"])
def test_head_stage_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    hd = head_of(case, "cuda")
    h = hd.desc()
    inp = inputs_of(case, "cuda")
    (_teacher_chain if case.kind == "chain" else _stage)(case, hd, h, inp)


FREE_BAR = 1e-3
# the free-running figure: rel RMS of a 20-step sample (64 values) against ref_sampler in fp64.  What separates the two: c rounds to the other
# bf16 neighbour on ~2e-4 of its elements (2^-8 each: 2^-8 sqrt(2e-4) = 5e-5 of a modulation row's inputs), fp32 arithmetic (1e-6 per stage), both
# carried through 20 steps x 4 layers; the solver contracts (cx < 1), so the sum stays near 1e-4.  1e-3, twenty times under the 2e-2 of the older
# whole-sample test; held on the CPU to >= 8 x the fp32 stand-in's distance.  No listed fault belongs to this figure.


def test_free_running_bar_sits_above_the_floor():
    hd = HeadData(1536, 64, 1536, 4, 512, seed=5)
    g = torch.Generator().manual_seed(11)
    cond, noise, temb = torch.randn(2, 1536, generator=g), torch.randn(64, generator=g), 0.5 * torch.randn(20, 1536, generator=g)
    coefs = production_coefs()
    ref = ref_sampler(hd, cond, noise, temb, coefs, 1.3)
    floor = _rel(ref_sampler(hd, cond, noise, temb, coefs, 1.3, torch.float32), ref)
    assert bool(torch.isfinite(ref).all()) and FREE_BAR >= FLOOR_HEADROOM * floor, floor


@pytest.mark.gpu
@pytest.mark.parametrize("cid", ["free_1p5b", "free_7b"])
def test_free_running_sample_vs_fp64(cid):
    """a 20-step sample with the production schedule's coefficients against the fp64 whole-sampler reference"""
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    hd = head_of(case, "cuda")
    h, inp = hd.desc(), inputs_of(case, "cuda")
    coefs = production_coefs(case.n)
    _, lat1, _ = call_sampler(case, hd, h, inp, case.n, coefs, cfg=1.3)
    _, lat2, _ = call_sampler(case, hd, h, inp, case.n, coefs, cfg=1.3)
    assert _same_bits(lat1, lat2)
    ref = ref_sampler(hd, inp["cond"], inp["noise"][0], inp["temb"], coefs, 1.3)
    e = _rel(lat1[0], ref)
    print(f"{cid}: free-running 20-step sample, rel RMS against fp64 {e:.2e}")
    _note("free-running " + cid[5:], FREE_BAR, e)
    assert e < FREE_BAR, (cid, e)


@pytest.mark.gpu
def test_sde_noise_in_state_space():
    """head_sde_proj<bf16>: NX of (utterance b, step i) sits at b * n_steps + i, its copied part exact, with ld_sde > n_steps * latent"""
    _need_gpu()
    case = CASES[CASE_IDS.index("bnd_b3_sde")]
    hd = head_of(case, "cuda")
    h, inp = hd.desc(), inputs_of(case, "cuda")
    region, _, _ = call_sampler(case, hd, h, inp, case.n, coef_rows(case.n, "chain", True))
    D, lat, n = case.D, case.latent, case.n
    NX = region("NX", (case.B * n, D + lat))
    P = hd.noisy_proj.double().cpu()
    for b in range(case.B):
        for i in range(n):
            nz = inp["sde"][b, i * lat:(i + 1) * lat].cpu()
            assert _same_bits(NX[b * n + i, D:], nz), (b, i)
            e = vec_errors(NX[b * n + i, :D], P @ nz.double())
            _note("x0", BAR["x0"], *e)
            assert e[0] < BAR["x0"][0] and e[1] < BAR["x0"][1], (b, i, e)


@pytest.mark.gpu
def test_zz_report():
    _need_gpu()
    path = os.environ.get("VV_HEAD_PARITY_OUT")
    lines = [f"{'class':<30} {'checks':>6} {'bar':>18} {'largest / bar':>14} {'bar / largest':>14}"]
    for k in sorted(_MEASURED):
        bar, cnt, worst = _MEASURED[k]
        lines.append(f"{k:<30} {cnt:>6} {str(bar):>18} {worst:>14.3f} {1 / max(worst, 1e-300):>14.1f}")
    print("\n".join(lines))
    if path and _MEASURED:
        with open(path, "w") as f:
            f.write(f"{torch.cuda.get_device_name(0)} (tests/test_hip_head_stages.py)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__" and "--table" in sys.argv:
    print(kernel_table())

// vv_gemv_rows.hip — the weight-streaming GEMV for 3 .. 8 activation rows (dialogues batched into the row dimension: rows = {positive,
// negative} x 2 .. 4 dialogues), on the matrix cores; and its 9 .. 16-row form (5 .. 8 dialogues) on the fragment-major bf16 copy, gemv_rows16_kernel.
//
// Roofline: HBM.  The VALU GEMV (vv_gemv_stream.hip) keeps M x K/wave activations in registers and spends M FMAs per weight: its time grows
// 1.2 - 1.6 us per row and M = 8 does not fit its registers at all for K > 1024.  Here one v_mfma_f32_16x16x32_bf16 consumes a wave's 1 KB
// weight load (16 weight rows x 32 k, 16 bytes per lane, straight to registers: nothing is shared between waves) against a 16-row activation
// fragment whose rows 0 .. 7 are the bf16 HIGH parts and rows 8 .. 15 the bf16 LOW parts of the 8 fp32 activation rows (hi + lo reproduces
// the fp32 value to 2^-17; weights are bf16, products and sums fp32): the cost per weight byte does not depend on the row count.
//
//   weights             row-major [N, K], or - VV_LIN_W_FRAG - the fragment-major copy [N / 16][K / 32][64 lanes][8]: lane (n = lane & 15,
//                       c = lane >> 4) of k step j of row group g finds W[16 g + n][32 j + 8 c ..+8] at ((g * K/32 + j) * 64 + lane) * 8, so
//                       one wave instruction reads 1 KB of contiguous memory and a wave's steps are one contiguous run.  From the row-major
//                       matrix the same instruction gathers 16 rows x 64 B (measured: 16.9 vs 14.0 us on the head's SwiGLU GEMV, 24.1 vs
//                       18.4 us on the LLM's, tools/mb_rows8.py).
//   fp8 weights         (VV_FP8 + VV_LIN_W_FRAG, weight-only) the e4m3fn codes in the fragment-major copy [N / 16][K / 64][64 lanes][16 B]: lane
//                       (n, c) of 64-wide k step j of row group g finds W[16 g + n][64 j + 8 c ..+8] in bytes 0 .. 7 and W[16 g + n][64 j + 32 + 8 c ..+8]
//                       in bytes 8 .. 15 at ((g * K/64 + j) * 64 + lane) * 16: one 1 KB wave load carries the B fragments of two 32-wide k steps.  The
//                       codes are decoded to bf16 in registers with the lane's row scale folded in (v_cvt_scalef32_pk_bf16_fp8; a power of two, so
//                       code * scale is exact in bf16) and meet the same hi / lo activation fragments on the same bf16 MFMA: the products and their
//                       summation order are those of the bf16 kernel on the effective matrix code * scale, bit for bit.
//   MXFP4 weights       (VV_MXFP4_FRAG, weight-only OCP MXFP4: the row-batched decode step and the serving sessions of a weight_quant="mxfp4" model)
//                       codes [N / 16][K / 128][64 lanes][16 B]: dword h of lane 16 c + n of 128-wide step J of row group g holds
//                       W[16 g + n][128 J + 32 h + 8 c + i] in nibble i (bits 4 i .. 4 i + 3) - the B fragment of 32-wide k step 4 J + h in the lane
//                       assignment of the bf16 fragment-major layout, so one 1 KB wave load carries FOUR MFMA steps.
//     scales            bytes [N / 16][K / 128][16 rows][4 B]: byte h of the dword at ((g * K/128 + J) * 16 + n) * 4 is the E8M0 byte of block 4 J + h of
//                       row 16 g + n.  An MX block (32 consecutive k of a row) is exactly one MFMA k step: one scale per B fragment, one 4-byte load
//                       per lane per weight load, no table, no LDS on the decode path.
//     decode            per dword h: s = 2^(e_h - 127) built as __uint_as_float(e_h << 23); four v_cvt_scalef32_pk_bf16_fp4 (byte select 0 .. 3) give
//                       the bf16x8 B fragment; value(code) * s is exact in bf16, so the products and their summation order are those of the bf16 kernel
//                       on the effective matrix wherever both cut K alike.
//     KS                128-wide weight loads per wave: 4 KS A fragments (16 KS VGPRs) against 4 KS VGPRs of codes - a 4-bit weight needs four times
//                       the activation registers and LDS per weight byte the bf16 form needs, which is what bounds KS (<= 4) and the K slice.
//   workgroup (g, s)    = 16 weight rows (row group g)  x  K slice s of `ksplit`;  its NW waves split the slice into `spw` weight loads each (32-wide
//                       k steps; 64-wide for fp8, 128-wide for MXFP4)
//   prologue            the block's x slice [8, K / ksplit] is fetched once (fp32), RMSNorm statistics over the block's columns, norm weight and
//                       adaLN shift / scale applied, split into hi / lo and laid out in LDS in fragment order; every wave then holds its A
//                       fragments in registers.  All of it is REQUESTED before the weights (loads return in order) and computed while the
//                       weights are in flight.
//   ksplit == 1         (K <= 2048) a block owns whole rows; with more row groups than resident blocks (the SwiGLU shapes) the blocks are
//                       persistent: they keep their fragments and walk row groups g, g + grid, ... with the next group's weights in flight.
//   ksplit > 1          long K with few rows (N = 1536: 96 row groups) cannot fill 256 CUs by row groups alone: the K slices of one row group
//                       meet through write-through partial tiles and a ticket; the last-arriving block folds them in a fixed order
//                       (deterministic) with all partial loads in flight at once, multiplies by rstd (RMSNorm is a per-row scalar: the
//                       slices accumulate the un-normalised x * norm_w and each contributes its partial sum of squares) and runs the epilogue.
//                       No release / acquire fences: the partials are sc1 stores and sc1 loads (cdna_hip_programming.md, in-launch split-K
//                       reduction); an agent-scope release per block (an L2 write-back each) cost 5 - 20 us per launch with 400 - 800 blocks.
//   epilogue            bias / GELU / SwiGLU / per-row or per-channel gate / residual, one output per thread, operands requested up front.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"
#include "vv_gemv_rows.h"

namespace {

// RowsAux, MAXSPLIT, the weight formats WF_* and rows_fpl, fp8_frags: vv_gemv_rows.h (shared with vv_gemv_rows_mx6.hip)

// The text of both kernels below (vv_gemv_rows_body.inc): KS weight loads per wave against KA = rows_fpl(WF) * KS activation fragments per row tile.  RT row tiles of 8
// activation rows each: every B fragment meets RT A fragments (tile t = the hi / lo parts of rows 8 t .. 8 t + 7), RT MFMAs per weight load.
//   RT == 1   gemv_rows_kernel, 3 .. 8 rows
//   RT == 2   gemv_rows16_kernel, 9 .. 16 rows: twice the fragments (LDS, registers), accumulators, epilogue threads (256) and partial tile; the
//             adaLN rows of tile 1 are requested once tile 0 is laid out (their registers are tile 0's), behind the weights; a wave adds the hi
//             and lo accumulator rows across its lane halves before they go to LDS (the same sum, in the same order, as the 8-row reduction
//             reads: the tile's 16 x 16 floats become 8 x 16), which keeps the widest instantiation inside one CU's LDS
// 3 .. 8 activation rows: one row tile
template <bool DUAL, int NW, int KS, bool PERS, int WF>
__global__ __launch_bounds__(NW * 64) void gemv_rows_kernel(const vv_lin_args a, const RowsAux x) {
  constexpr int RT = 1;
#include "vv_gemv_rows_body.inc"
}

// 9 .. 16 activation rows on the fragment-major bf16 copy: two row tiles, two MFMAs per weight load, one pass over the weights
template <bool DUAL, int NW, int KS, bool PERS>
__global__ __launch_bounds__(NW * 64) void gemv_rows16_kernel(const vv_lin_args a, const RowsAux x) {
  constexpr int RT = 2, WF = WF_BF16;
#include "vv_gemv_rows_body.inc"
}

int g_rows_on = 1;          // tuning hook "gemv_rows": 0 = never take this path
int g_rows_blocks = 448;    // row groups x K slices aimed for before the K split stops growing
int g_rows_pers = 192;      // persistent blocks of the whole-row SwiGLU kernels: each block's activation prologue is 150 KB of L2 reads, so FEWER blocks
                            // than CUs win (head: 11.05 us at 144 blocks, 11.65 at 256, 15.2 at 288 one-shot blocks; LLM: 15.7 at 187, 16.9 at 256)
int g_rows_dbg = 0;
int g_rows_atomic = 1;      // tuning hook "gemv_rows_atomic": 0 = always fold K slices through the ticket (deterministic summation order)

template <bool DUAL, int NW, int KS, bool PERS, int WF>
int launch_cfg(const vv_lin_args& a, const RowsAux& x, int gx, hipStream_t s) {
  const size_t lds = (size_t)NW * rows_fpl(WF) * KS * 64 * 16;    // the LDS limit of every instantiation is raised in vv_gemv_rows_init (not capturable)
  hipLaunchKernelGGL((gemv_rows_kernel<DUAL, NW, KS, PERS, WF>), dim3(gx, x.ksplit), dim3(NW * 64), lds, s, a, x);
  return 1;
}

template <bool DUAL, int NW, int KS, bool PERS>
int launch_cfg16(const vv_lin_args& a, const RowsAux& x, int gx, hipStream_t s) {
  const size_t lds = (size_t)2 * NW * KS * 64 * 16;               // two row tiles of fragments; raised in vv_gemv_rows_init as well
  hipLaunchKernelGGL((gemv_rows16_kernel<DUAL, NW, KS, PERS>), dim3(gx, x.ksplit), dim3(NW * 64), lds, s, a, x);
  return 1;
}

// Every kernel of this file, as (dual, nw, ks, pers, wf) - exactly what vv_gemv_rows_decide can choose: per format the whole-row kernels (8 waves;
// SwiGLU also persistent), the SwiGLU K split (the same one-shot kernels) and the single-matrix K split (4 waves)
#define VV_ROWS_ALL(X)                                                                                                         \
  X(0, 8, 4, 0, WF_BF16) X(0, 8, 6, 0, WF_BF16) X(0, 8, 8, 0, WF_BF16)                                                         \
  X(1, 8, 4, 0, WF_BF16) X(1, 8, 6, 0, WF_BF16) X(1, 8, 8, 0, WF_BF16) X(1, 8, 4, 1, WF_BF16) X(1, 8, 6, 1, WF_BF16)           \
  X(0, 4, 3, 0, WF_BF16) X(0, 4, 6, 0, WF_BF16) X(0, 4, 9, 0, WF_BF16) X(0, 4, 12, 0, WF_BF16)                                 \
  X(0, 8, 2, 0, WF_FP8) X(0, 8, 4, 0, WF_FP8)                                                                                  \
  X(1, 8, 2, 0, WF_FP8) X(1, 8, 4, 0, WF_FP8) X(1, 8, 2, 1, WF_FP8) X(1, 8, 4, 1, WF_FP8)                                      \
  X(0, 4, 2, 0, WF_FP8) X(0, 4, 4, 0, WF_FP8) X(0, 4, 6, 0, WF_FP8) X(0, 4, 8, 0, WF_FP8)                                      \
  X(0, 8, 1, 0, WF_MXFP4) X(0, 8, 2, 0, WF_MXFP4)                                                                              \
  X(1, 8, 1, 0, WF_MXFP4) X(1, 8, 2, 0, WF_MXFP4) X(1, 8, 1, 1, WF_MXFP4) X(1, 8, 2, 1, WF_MXFP4)                              \
  X(0, 4, 1, 0, WF_MXFP4) X(0, 4, 2, 0, WF_MXFP4) X(0, 4, 3, 0, WF_MXFP4) X(0, 4, 4, 0, WF_MXFP4)

// Every gemv_rows16_kernel, as (dual, nw, ks, pers): the bf16 forms of the list above, chosen by the same rules
#define VV_ROWS16_ALL(X)                                                                       \
  X(0, 8, 4, 0) X(0, 8, 6, 0) X(0, 8, 8, 0)                                                    \
  X(1, 8, 4, 0) X(1, 8, 6, 0) X(1, 8, 8, 0) X(1, 8, 4, 1) X(1, 8, 6, 1)                        \
  X(0, 4, 3, 0) X(0, 4, 6, 0) X(0, 4, 9, 0) X(0, 4, 12, 0)

// the decision's template choice: gemv_rows_kernel<dual, nw, ks, pers, wf> (r.rt == 2: gemv_rows16_kernel<dual, nw, ks, pers>) and its grid
void rows_cfg(vv_rows_route& r, int dual, int nw, int ks, int pers, int wf) {
  r.dual = dual; r.nw = nw; r.ks = ks; r.pers = pers; r.wf = wf;
  r.gx = r.n_groups;
  if (pers && r.gx > g_rows_pers) {                     // the same number of row groups for every block
    const int per = (r.n_groups + g_rows_pers - 1) / g_rows_pers;
    r.gx = (r.n_groups + per - 1) / per;
  }
  r.kind = 1;
}

// The K split of a long row (`steps` weight loads, NW waves per block), for every format: the first split whose waves take <= kscap loads and that
// gives g_rows_blocks workgroups (or leaves <= `few` loads per wave), else the first with <= ksmax loads.  Sets r.ksplit, r.spw and r.atomic;
// false = no split within MAXSPLIT, or the fold needs a workspace that is not there.
bool rows_split(const vv_lin_args& a, int steps, int n_groups, int NW, int kscap, int ksmax, int few, bool have_ws, size_t part_floats,
                size_t n_tickets, vv_rows_route& r) {
  const bool dual = a.w2 != nullptr;
  const int maxsplit = MAXSPLIT / r.rt;               // two row tiles: partial tiles twice the size, half as many of them
  int ksplit = 0, spw = 0;
  for (int sp = 2; sp <= maxsplit && !ksplit; ++sp) {
    const int w = (steps + sp * NW - 1) / (sp * NW);
    if (w <= kscap && ((long)n_groups * sp >= g_rows_blocks || w <= few)) { ksplit = sp; spw = w; }
  }
  for (int sp = 2; sp <= maxsplit && !ksplit; ++sp) {
    const int w = (steps + sp * NW - 1) / (sp * NW);
    if (w <= ksmax) { ksplit = sp; spw = w; }
  }
  if (!ksplit) return false;
  while (ksplit > 1 && (ksplit - 1) * NW * spw >= steps) --ksplit;     // drop K slices that would start past the end
  const size_t pst = (size_t)(dual ? 264 : 136) * r.rt;
  r.atomic = g_rows_atomic && !dual && a.pro == VV_PRO_NONE && a.act == VV_ACT_NONE && a.res && a.res == a.out && a.ldres == a.ldo;
  if (!r.atomic && (!have_ws || (size_t)n_groups * ksplit * pst > part_floats || (size_t)n_groups > n_tickets)) return false;
  r.ksplit = ksplit; r.spw = spw;
  return true;
}

// The smallest built KS that holds spw loads per wave.  wide: the 8-wave kernels (whole rows, SwiGLU K split); else the 4-wave single-matrix K split.
int rows_ks(int wf, bool wide, int spw) {
  if (wf == WF_MXFP4 || wf == WF_MXFP6) return spw;     // every KS the decision can ask for is built (MXFP6: the decision asks vv_gemv_rows_mx6_built)
  if (wf == WF_FP8) return spw <= 2 ? 2 : spw <= 4 || wide ? 4 : spw <= 6 ? 6 : 8;
  if (wide) return spw <= 4 ? 4 : spw <= 6 ? 6 : 8;
  return spw <= 3 ? 3 : spw <= 6 ? 6 : spw <= 9 ? 9 : 12;
}

}  // namespace

void vv_gemv_rows_set_dbg(int d) { g_rows_dbg = d; }
void vv_gemv_rows_set_atomic(int on) { g_rows_atomic = on; }
void vv_gemv_rows_set(int on, int blocks, int pers) {
  if (on >= 0) g_rows_on = on;
  if (blocks > 0) g_rows_blocks = blocks;
  if (pers > 0) g_rows_pers = pers;
}

// floats of partials workspace a launch on (n, k, dual) may need (upper bound over the launcher's rules), and ticket ints.  The 16-row kernel
// needs no more: its partial tiles are twice the 8-row kernel's and it splits K at most MAXSPLIT / 2 ways
size_t vv_gemv_rows_part_floats(int n, int dual) { return (size_t)((n + 15) / 16) * MAXSPLIT * (dual ? 264 : 136); }
size_t vv_gemv_rows_tickets(int n) { return (size_t)((n + 15) / 16); }

// every kernel's LDS attribute is set before any graph capture (hipFuncSetAttribute is not capturable)
int vv_gemv_rows_init() {
#define VV_ROWS_ATTR(D, NW, KS, P, WF)                                                                                                       \
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_rows_kernel<(D != 0), NW, KS, (P != 0), WF>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                          NW * rows_fpl(WF) * KS * 64 * 16) != hipSuccess)                                                                \
    return vv_set_error(VV_E_HIP, "gemv_rows: cannot raise the dynamic LDS limit");
  VV_ROWS_ALL(VV_ROWS_ATTR)
#undef VV_ROWS_ATTR
#define VV_ROWS16_ATTR(D, NW, KS, P)                                                                                                         \
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_rows16_kernel<(D != 0), NW, KS, (P != 0)>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                          2 * NW * KS * 64 * 16) != hipSuccess)                                                                           \
    return vv_set_error(VV_E_HIP, "gemv_rows16: cannot raise the dynamic LDS limit");
  VV_ROWS16_ALL(VV_ROWS16_ATTR)
#undef VV_ROWS16_ATTR
  return vv_gemv_rows_mx6_init();      // gemv_rows_mx6_kernel (vv_gemv_rows_mx6.hip)
}

// The one copy of what a call on this unit's weight-only formats must be (vv_common.h): fragment-major fp8 codes and VV_MXFP4_FRAG, 3..8 fp32 rows,
// whole row groups and weight loads, scales for every matrix; an fp8 call outside that names a layout that does not exist (VV_E_ARG).  What
// bf16 calls need too (aligned operands, a row pitch) stays with the decision below.
const char* vv_gemv_rows_refusal(const vv_lin_args& a, int* rc) {
  const bool fp8 = a.wdt == VV_FP8;
  const char* lacks = nullptr;
  if (!fp8 && a.wdt != VV_MXFP4_FRAG) return "VV_FP8 or VV_MXFP4_FRAG weights";
  if (a.flags & (VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) lacks = "fp32 activations and outputs (no bf16 hand-off)";
  else if (a.m < 3 || a.m > 8) lacks = "3..8 rows";
  else if (a.n < 16 || a.n % 16) lacks = "n % 16 == 0";
  else if (a.k % (fp8 ? 64 : 128)) lacks = fp8 ? "k % 64 == 0" : "k % 128 == 0";
  else if (!a.wscale || (a.w2 && !a.w2scale)) lacks = fp8 ? "wscale (w2scale)" : "scale bytes for w (and w2)";
  if (lacks) { if (fp8 && rc) *rc = VV_E_ARG; return lacks; }
  if (!(a.flags & VV_LIN_W_FRAG)) return "VV_LIN_W_FRAG (the fragment-major copy)";
  if (!fp8 && ((uintptr_t)a.wscale % 4 || (a.w2 && (uintptr_t)a.w2scale % 4))) return "4-byte aligned scale bytes";
  return nullptr;
}

// The decision: which instantiation the call takes, its K split and grid; kind 0 = not covered (the caller falls back).  have_ws: a split-K
// workspace of part_floats floats and n_tickets tickets exists (without one only shapes that need no K split, or the atomic form, are taken).
// fp8, MXFP4 and MXFP6 weights: fragment-major only (VV_LIN_W_FRAG).  Reads the arguments' values and alignments and the tune state only.
//
// The formats share the pattern and differ in the width of a weight load (32, 64, 128 k) and in what a load costs in registers:
//   bf16    4 VGPRs per load and matrix, 4 of activation fragment: 8 loads hold the whole K <= 2048 row in 8 waves; the single-matrix split-K
//           form goes up to 12 loads per wave.
//   fp8     a 64-wide load costs 4 VGPRs per matrix (8 in flight per persistent buffer pair) and its two activation fragments 8: KS = 4 holds the
//           whole row and leaves the persistent dual form 64 weight + 32 fragment VGPRs, so fp8 runs persistent at every whole-row width; the
//           single-matrix split-K form goes up to 8 loads (8 KB in flight per wave, as the bf16 form's 8 - 12).
//   MXFP6   (VV_MXFP6_FRAG, the kernels of vv_gemv_rows_mx6.hip) MXFP4's rules: a 128-wide load costs 6 VGPRs of codes + 1 of scale bytes per matrix
//   MXFP4   a 128-wide load costs 4 VGPRs of codes + 1 of scale bytes per matrix and 16 of activation fragments, and 4 KB of LDS per wave: two loads
//           hold the whole row (one chunk per thread: the adaLN prologue fits), the single-matrix split-K form goes up to 4 loads per wave
//           (64 fragment VGPRs, 64 KB of LDS per block).
vv_rows_route vv_gemv_rows_decide(const vv_lin_args& a, bool have_ws, size_t part_floats, size_t n_tickets) {
  vv_rows_route r = {};
  const int wf = a.wdt == VV_BF16 ? WF_BF16 : a.wdt == VV_FP8 ? WF_FP8 : a.wdt == VV_MXFP4_FRAG ? WF_MXFP4 : a.wdt == VV_MXFP6_FRAG ? WF_MXFP6 : -1;
  if (!g_rows_on || wf < 0 || a.m < 3 || a.m > 16) return r;
  if (wf != WF_BF16 && (wf == WF_MXFP6 ? vv_gemv_rows_mx6_refusal(a, nullptr) : vv_gemv_rows_refusal(a, nullptr))) return r;
  r.rt = a.m > 8 ? 2 : 1;                             // 9 .. 16 rows: gemv_rows16_kernel, on the fragment-major bf16 copy only
  if (r.rt == 2 && !(a.flags & VV_LIN_W_FRAG)) return r;
  const int kw = 32 * rows_fpl(wf);                   // k per weight load
  if (a.k % kw || a.k < kw) return r;
  if (a.pro == VV_PRO_SILU || (a.flags & (VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) || a.ldx == 0) return r;
  if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16) || (uintptr_t)a.x % 16 || a.ldx % 4) return r;
  if (a.norm_w && (uintptr_t)a.norm_w % 16) return r;
  if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return r;
  if (wf == WF_BF16 && (a.flags & VV_LIN_W_FRAG) && a.n % 16) return r;
  const bool dual = a.w2 != nullptr;
  const int steps = a.k / kw, n_groups = (a.n + 15) / 16;
  r.n_groups = n_groups; r.atomic = 0;
  // whole rows per block when K <= 2048 (8 waves x <= 8 bf16 loads): no cross-block reduction at all
  if (a.k <= 2048) {
    r.ksplit = 1;
    r.spw = (steps + 7) / 8;
    // persistent when the row groups outnumber the blocks aimed for; bf16: 8 steps x 2 matrices x 2 buffers do not fit the registers
    const bool pers = dual && n_groups > g_rows_pers && (wf != WF_BF16 || r.spw <= 6);
    rows_cfg(r, dual, 8, rows_ks(wf, true, r.spw), pers, wf);
    if (wf == WF_MXFP6 && !vv_gemv_rows_mx6_built(r.dual, r.nw, r.ks, r.pers)) r.kind = 0;
    return r;
  }
  // long rows: K slices across blocks, folded by the last arriver
  if (a.mod_scale) return r;                          // the modulated prologue needs the whole row's statistic up front
  // loads per wave the split aims for and accepts at most, [format][dual], and the few loads below which more blocks are not worth another slice
  static const int KSCAP[4][2] = {{9, 8}, {6, 4}, {3, 2}, {3, 2}}, KSMAX[4][2] = {{12, 8}, {8, 4}, {4, 2}, {4, 2}}, FEW[4] = {3, 2, 1, 1};
  const int NW = dual ? 8 : 4;
  if (!rows_split(a, steps, n_groups, NW, KSCAP[wf][dual], KSMAX[wf][dual], FEW[wf], have_ws, part_floats, n_tickets, r)) return r;
  rows_cfg(r, dual, NW, rows_ks(wf, dual, r.spw), 0, wf);
  if (wf == WF_MXFP6 && !vv_gemv_rows_mx6_built(r.dual, r.nw, r.ks, r.pers)) r.kind = 0;
  return r;
}

// The launch of a decided route: 1 = launched, 0 = r.kind == 0 or an instantiation that is not built.  part / tickets: the split-K workspace
// the decision was told about (tickets zeroed by the caller once; every launch leaves them zero) or null.
int vv_launch_gemv_rows_route(const vv_lin_args& a, const vv_rows_route& r, float* part, int* tickets, hipStream_t s) {
  if (r.kind != 1) return 0;
  if (r.wf == WF_MXFP6) return vv_launch_gemv_rows_mx6_route(a, r, part, tickets, s);      // the kernels of vv_gemv_rows_mx6.hip
  RowsAux x;
  x.part = part; x.tickets = tickets; x.dbg = g_rows_dbg; x.n_groups = r.n_groups; x.atomic = r.atomic; x.ksplit = r.ksplit; x.spw = r.spw;
  if (r.rt == 2) {
#define VV_ROWS16_CASE(D, NW, KS, P) \
    if (r.dual == D && r.nw == NW && r.ks == KS && r.pers == P && r.wf == WF_BF16) return launch_cfg16<(D != 0), NW, KS, (P != 0)>(a, x, r.gx, s);
    VV_ROWS16_ALL(VV_ROWS16_CASE)
#undef VV_ROWS16_CASE
    return 0;
  }
#define VV_ROWS_CASE(D, NW, KS, P, WF) \
  if (r.dual == D && r.nw == NW && r.ks == KS && r.pers == P && r.wf == WF) return launch_cfg<(D != 0), NW, KS, (P != 0), WF>(a, x, r.gx, s);
  VV_ROWS_ALL(VV_ROWS_CASE)
#undef VV_ROWS_CASE
  return 0;
}

// the name vv_linear_route reports for this file's route: spelled here and nowhere else
int vv_gemv_rows_route_name(const vv_rows_route& r, char* name, int cap) {
  if (r.rt == 2)
    return snprintf(name, (size_t)cap, "gemv_rows16<dual=%d,nw=%d,ks=%d,pers=%d> ksplit=%d atomic=%d", r.dual, r.nw, r.ks, r.pers, r.ksplit, r.atomic);
  if (r.wf == WF_MXFP6)
    return snprintf(name, (size_t)cap, "gemv_rows_mx6<dual=%d,nw=%d,ks=%d,pers=%d> ksplit=%d atomic=%d", r.dual, r.nw, r.ks, r.pers, r.ksplit, r.atomic);
  if (r.wf == WF_MXFP4)
    return snprintf(name, (size_t)cap, "gemv_rows_mx<dual=%d,nw=%d,ks=%d,pers=%d> ksplit=%d atomic=%d", r.dual, r.nw, r.ks, r.pers, r.ksplit, r.atomic);
  return snprintf(name, (size_t)cap, "gemv_rows<dual=%d,nw=%d,ks=%d,pers=%d,f8=%d> ksplit=%d atomic=%d", r.dual, r.nw, r.ks, r.pers, r.wf, r.ksplit, r.atomic);
}

// decide + launch: 1 launched, 0 not covered (the caller falls back), < 0 error
int vv_launch_gemv_rows(const vv_lin_args& a, float* part, size_t part_floats, int* tickets, size_t n_tickets, hipStream_t s) {
  return vv_launch_gemv_rows_route(a, vv_gemv_rows_decide(a, part && tickets, part_floats, n_tickets), part, tickets, s);
}

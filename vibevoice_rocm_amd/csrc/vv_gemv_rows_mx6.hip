// vv_gemv_rows_mx6.hip — the 3 .. 8-row matrix-core GEMV on VV_MXFP6_FRAG weights: the row-batched decode step and the serving sessions of a
// weight_quant="mxfp6" model (mxfp6_row_batch=True).  The kernel is the rows GEMV's (vv_gemv_rows.hip describes it: prologue requested ahead of the
// weights, whole-row / persistent SwiGLU / K-split forms, ticketed fold in a fixed order or the atomic form, vv_epi_value epilogue) - the same
// text, vv_gemv_rows_body.inc, as a fourth weight format WF_MXFP6.  It is a unit and a kernel name of its own so that the kernel set of
// vv_gemv_rows.hip stays the one its tests enumerate; the DECISION stays in vv_gemv_rows.hip too (vv_gemv_rows_decide: one copy of the thresholds
// for all four formats), which asks this file which instantiations exist and hands it the launch.
//
// What the format changes (layout: include/vv_hip.h, VV_MXFP6_FRAG):
//   block ownership     gfx950 decodes fp6 32 codes at a time - v_cvt_scalef32_pk32_bf16_fp6: six dwords and a float scale in, 32 bf16 out - so
//                       a lane owns a whole MX block (32 consecutive k of one row, 24 bytes): lane 16 c + n of 128-wide step J of row group g owns
//                       block 4 J + c of row 16 g + n.  Its 24 bytes come as one 16-byte and one 8-byte load from two planes, each contiguous
//                       and aligned across the wave (1 KB + 512 B), the scale dword of row n as one 4-byte load of which the lane takes byte c.
//   k order             the 32 decoded values are four B fragments: MFMA h takes elements 8 h .. 8 h + 7 of every lane's block, the k set
//                       {128 J + 32 c + 8 h + i}.  The activation fragments are laid out in LDS in that order (the prologue swaps the roles of
//                       the step h and the lane quarter c inside a 128-wide group), so every product meets its partner; the SUMMATION order is
//                       fixed but is not the bf16 kernel's: against the bf16 fragment-major form results agree to fp32 reassociation.
//   registers           per load and matrix 4 + 2 VGPRs of codes + 1 of scale bytes against 16 of activation fragments, and 16 transient for
//                       the decoded block: KS is bounded as for MXFP4 (<= 4 loads per wave in the single-matrix K split, <= 2 in the 8-wave
//                       kernels), the same instantiations, the same LDS (4 KB per wave and load).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"
#include "vv_gemv_rows.h"

namespace {

template <bool DUAL, int NW, int KS, bool PERS>
__global__ __launch_bounds__(NW * 64) void gemv_rows_mx6_kernel(const vv_lin_args a, const RowsAux x) {
  constexpr int RT = 1, WF = WF_MXFP6;
#include "vv_gemv_rows_body.inc"
}

// Every kernel of this file, as (dual, nw, ks, pers) - exactly what vv_gemv_rows_decide can choose for WF_MXFP6: the whole-row kernels (8 waves;
// SwiGLU also persistent), the SwiGLU K split (the same one-shot kernels) and the single-matrix K split (4 waves)
#define VV_ROWS_MX6_ALL(X)                                       \
  X(0, 8, 1, 0) X(0, 8, 2, 0)                                    \
  X(1, 8, 1, 0) X(1, 8, 2, 0) X(1, 8, 1, 1) X(1, 8, 2, 1)        \
  X(0, 4, 1, 0) X(0, 4, 2, 0) X(0, 4, 3, 0) X(0, 4, 4, 0)

constexpr size_t mx6_lds(int nw, int ks) { return (size_t)nw * rows_fpl(WF_MXFP6) * ks * 64 * 16; }

}  // namespace

// is gemv_rows_mx6_kernel<dual, nw, ks, pers> compiled?  The decision asks before it names a route
bool vv_gemv_rows_mx6_built(int dual, int nw, int ks, int pers) {
#define VV_MX6_IS(D, NW, KS, P) if (dual == D && nw == NW && ks == KS && pers == P) return true;
  VV_ROWS_MX6_ALL(VV_MX6_IS)
#undef VV_MX6_IS
  return false;
}

// every kernel's LDS attribute, set from vv_gemv_rows_init before any graph capture (hipFuncSetAttribute is not capturable)
int vv_gemv_rows_mx6_init() {
#define VV_MX6_ATTR(D, NW, KS, P)                                                                                                                 \
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_rows_mx6_kernel<(D != 0), NW, KS, (P != 0)>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                          (int)mx6_lds(NW, KS)) != hipSuccess)                                                                                 \
    return vv_set_error(VV_E_HIP, "gemv_rows_mx6: cannot raise the dynamic LDS limit");
  VV_ROWS_MX6_ALL(VV_MX6_ATTR)
#undef VV_MX6_ATTR
  return 0;
}

// The one copy of what a VV_MXFP6_FRAG call must be (vv_hip.h): NULL = taken so far (the decision may still find no kernel: k > 2048 without
// split-K scratch), else what the call lacks.  Every refusal is VV_E_UNSUPPORTED.  Values and alignments only.
const char* vv_gemv_rows_mx6_refusal(const vv_lin_args& a, int*) {
  if (a.wdt != VV_MXFP6_FRAG) return "VV_MXFP6_FRAG weights";
  if (a.flags & VV_LIN_W_MXGEMM) return "no VV_LIN_W_MXGEMM (there is no GEMM on the 6-bit codes)";
  if (a.flags & (VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) return "fp32 activations and outputs (no bf16 hand-off)";
  if (a.m < 3 || a.m > 8) return "3..8 rows";
  if (!(a.flags & VV_LIN_W_FRAG)) return "VV_LIN_W_FRAG (the fragment-major form is the only one this type has)";
  if (a.n < 16 || a.n % 16) return "n % 16 == 0";
  if (a.k % 128) return "k % 128 == 0";
  if (!a.wscale || (a.w2 && !a.w2scale)) return "scale bytes for w (and w2)";
  if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16)) return "16-byte aligned codes";
  if ((uintptr_t)a.wscale % 4 || (a.w2 && (uintptr_t)a.w2scale % 4)) return "4-byte aligned scale bytes";
  return nullptr;
}

// The launch of a route vv_gemv_rows_decide named for this file (r.wf == 3): 1 = launched, 0 = no such instantiation
int vv_launch_gemv_rows_mx6_route(const vv_lin_args& a, const vv_rows_route& r, float* part, int* tickets, hipStream_t s) {
  RowsAux x;
  x.part = part; x.tickets = tickets; x.dbg = 0; x.n_groups = r.n_groups; x.atomic = r.atomic; x.ksplit = r.ksplit; x.spw = r.spw;
#define VV_MX6_CASE(D, NW, KS, P)                                                                                                               \
  if (r.dual == D && r.nw == NW && r.ks == KS && r.pers == P) {                                                                                 \
    hipLaunchKernelGGL((gemv_rows_mx6_kernel<(D != 0), NW, KS, (P != 0)>), dim3(r.gx, r.ksplit), dim3(NW * 64), mx6_lds(NW, KS), s, a, x);      \
    return 1;                                                                                                                                   \
  }
  VV_ROWS_MX6_ALL(VV_MX6_CASE)
#undef VV_MX6_CASE
  return 0;
}

// vv_gemv_rows.h - what the kernel units that include vv_gemv_rows_body.inc share (vv_gemv_rows.hip, which describes the kernel, and
// vv_gemv_rows_mx6.hip): the launch's side argument, the weight formats and the fp8 decode.  Everything sits in an unnamed namespace: each
// unit's kernels keep the parameter type (and so the symbol names) they had when vv_gemv_rows.hip held these lines itself.
#ifndef VV_GEMV_ROWS_H
#define VV_GEMV_ROWS_H
#include "vv_device.h"

namespace {

struct RowsAux {
  int atomic;        // ksplit > 1 with a linear epilogue whose residual already sits in `out` (res == out): every K slice adds gate * (partial [+ bias])
                     // to out with fp32 atomics - no partial tiles, no ticket, nothing to wait for (the summation ORDER of the slices then varies from
                     // run to run: results reproduce to fp32 rounding, ~1e-7, not bit for bit; vv_tune("gemv_rows_atomic", 0) keeps the ticket)
  int dbg;           // timing experiments (wrong results; bf16 and fp8 only): 2 = no ticket merge, 4 = no activation loads
  float* part;       // [n_groups][ksplit][PST] partial tiles (ksplit > 1)
  int* tickets;      // [n_groups], zero on entry, left zero
  int ksplit, spw;   // K slices per row group; weight loads per wave (32-wide k steps, 64-wide for fp8, 128-wide for MXFP4 and MXFP6)
  int n_groups;
};

constexpr int MAXSPLIT = 16;

// 16 e4m3fn codes (one fp8 fragment-major lane load) -> the bf16 B fragments of two 32-wide k steps, times the row scale s (a power of two)
__device__ __forceinline__ void fp8_frags(const u32x4 w, float s, bf16x8& b0, bf16x8& b1) {
  bf16x2 p[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    p[2 * i] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], s, false);
    p[2 * i + 1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w[i], s, true);
  }
  b0 = bf16x8{p[0][0], p[0][1], p[1][0], p[1][1], p[2][0], p[2][1], p[3][0], p[3][1]};
  b1 = bf16x8{p[4][0], p[4][1], p[5][0], p[5][1], p[6][0], p[6][1], p[7][0], p[7][1]};
}

// The weight format WF (vv_rows_route.wf) owns the width of a weight load, the addresses `issue` computes, the decode in front of the MFMA, the
// scale registers of the persistent walk and - MXFP6 - the k order of the activation fragments; nothing else: prologue, LDS layout, fold, atomic
// form and epilogue are one text for all four.
constexpr int WF_BF16 = 0;      // row-major or fragment-major bf16: a load is one 32-wide k step
constexpr int WF_FP8 = 1;       // fragment-major e4m3fn codes, a row scale: a load is two 32-wide k steps
constexpr int WF_MXFP4 = 2;     // fragment-major e2m1 codes, a scale dword beside each load: a load is four 32-wide k steps
constexpr int WF_MXFP6 = 3;     // VV_MXFP6_FRAG: a lane's load is one whole MX block (16 + 8 bytes from two planes), a scale dword beside it: four MFMA steps
constexpr int rows_fpl(int wf) { return wf == WF_MXFP6 ? 4 : 1 << wf; }    // 32-wide A fragments per weight load

typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef __bf16 bf16x32 __attribute__((ext_vector_type(32)));

// One MX block of e2m3 codes (24 bytes: 16 from plane A, 8 from plane B; code i in bits 6 i .. 6 i + 5) under scale byte e -> its 32 bf16 weights
__device__ __forceinline__ bf16x32 mx6_block(const u32x4 lo, const u32x2 hi, unsigned e) {
  const u32x6 c = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y};
  return __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(c, __uint_as_float(e << 23));
}

}  // namespace

#endif

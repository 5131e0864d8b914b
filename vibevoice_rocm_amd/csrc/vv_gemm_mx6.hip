// vv_gemm_mx6.hip — the matrix-core GEMM on MXFP6 (e2m3) CODES: the prompt prefill and every other non-decode pass of 3 or more rows of a lean
// weight_quant="mxfp6" model (no bf16 copy of the matrix exists), reached through VV_LIN_W_MX6GEMM with wdt == VV_MXFP6 only.  The counterpart of
// vv_gemm_mx.hip (MXFP4), with the same contract:
//   out[m, n] = epilogue(sum_k W_eff[n, k] * x[m, k])        m >= 3, n % 16 == 0, k % 128 == 0, x bf16 (VV_LIN_X_BF16, no prologue)
//   W_eff[n, k] = value(code) * 2^(e - 127), W in the VV_MXFP6 companion layout (pack_mxfp6, include/vv_hip.h): exact in bf16
// The weights never pass through LDS, a lookup table or memory in decoded form.  gfx950 decodes fp6 a whole MX block at a time
// (v_cvt_scalef32_pk32_bf16_fp6, mx6_block of vv_gemv_rows.h), so a LANE OWNS A BLOCK: lane 16 c + n of 128-wide step J of a 16-channel group
// takes block 4 J + c of row n of the group - 16 bytes of the row group's plane A, 8 bytes of its plane B and the dword that holds the block's
// E8M0 bytes of the group's four rows, of which the lane uses byte n % 4.  A wave load is 16 segments of 64 bytes (plane A), 16 of 32 bytes
// (plane B) and 16 of 16 bytes (scales).  The 32 decoded values are the A fragments of four MFMAs: MFMA h takes elements 8 h .. 8 h + 7 and so
// meets k = 128 J + 32 c + 8 h + i, against the activation piece 4 c + h of the slab (vv_gemm_mx.hip reads piece 4 s + c: the permuted k order
// changes which 16-byte piece a lane reads and nothing else).  In the accumulators a lane holds, for one activation row, the 4 CONSECUTIVE
// channels 4 (lane / 16) + e of the group: the epilogue is one float4 (uint2) per row tile and group with no shuffle.
// A workgroup owns 64 rows x (32 MX6_CG) channels: 4 waves sit 2 (channels) x 2 (rows), each with MX6_CG channel groups of 16 and 2 row tiles of
// 16; a wave reads its 8 activation fragments of a slab from LDS once and uses each for MX6_CG (SwiGLU: 2 MX6_CG) MFMAs.  The activations go
// global -> LDS by LDS-DMA as in vv_gemm_mx.hip (128-k slabs, two buffers, the bank swizzle on the source address: slot s of row r holds k piece
// s ^ (r & 15)); the codes of slab t + 1 are requested into registers while the matrix cores work on slab t.
// Determinism: no atomics, no split K - every output element is one fp32 accumulator that meets the 128-wide steps in ascending order and
// h = 0 .. 3 in order inside a step, each an MFMA whose result for one element depends on that element's weight row and activation row alone.
// A row's result therefore does not depend on m, on the row's place in the call or on the other rows (tests/test_hip_gemm_mx6.py holds this
// bit for bit).  Measured tile variants and timings: profiles/mxfp6_lean.txt.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <type_traits>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"
#include "vv_gemv_rows.h"

#ifndef VV_MX6_CG
#define VV_MX6_CG 2                               // 16-channel groups per wave: the shipped tile is 64 rows x 64 channels (profiles/mxfp6_lean.txt)
#endif

namespace {

constexpr int MX6_CG = VV_MX6_CG;
constexpr int MX6_TM = 64;                        // rows of a workgroup's tile
constexpr int MX6_TN = 2 * MX6_CG * 16;           // channels of a workgroup's tile: 2 waves x MX6_CG groups x 16 rows
constexpr int MX6_BK = 128;                       // K elements per slab: a row is 256 bytes = 16 pieces of 16; one block per lane, four MFMA steps
constexpr int MX6_SLAB = MX6_TM * MX6_BK * 2;     // bytes of one activation slab (16 KB)
constexpr int MX6_PIECES = MX6_SLAB / (16 * 256); // DMA instructions per thread per slab (4)
constexpr int MX6_RT = 2;                         // 16-row tiles per wave

// one slab's blocks of one matrix, as a lane holds them: per channel group 16 + 8 code bytes and the scale dword of the block's row group
struct Mx6W { u32x4 a[MX6_CG]; u32x2 b[MX6_CG]; unsigned e[MX6_CG]; };

template <bool DUAL, bool OBF>
__global__ __launch_bounds__(256) void gemm_mx6_kernel(const vv_lin_args a) {
  __shared__ __attribute__((aligned(16))) unsigned char xsm[2 * MX6_SLAB];    // [2 buffers][64 rows][16 slots of 16 bytes]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.m, K = a.k, N = a.n;
  const int mtiles = (M + MX6_TM - 1) / MX6_TM;
  const int wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int n0 = (wg / mtiles) * MX6_TN, m0 = (wg % mtiles) * MX6_TM;        // consecutive workgroups share the weight panel
  // piece p = 256 i + tid of a slab: LDS row p >> 4, slot p & 15 <- the row's k piece (p & 15) ^ (row & 15)
  const bf16_t* xg[MX6_PIECES];
#pragma unroll
  for (int i = 0; i < MX6_PIECES; ++i) {
    const int p = 256 * i + tid, row = p >> 4, kp = (p & 15) ^ (row & 15);
    xg[i] = reinterpret_cast<const bf16_t*>(a.x) + (int64_t)min(m0 + row, M - 1) * a.ldx + kp * 8;       // rows past M: a valid row, masked at the store
  }
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto stage = [&](int buf, int k0) {
    unsigned char* base = xsm + buf * MX6_SLAB + wave * 1024;                // wave-uniform: the DMA adds lane * 16
#pragma unroll
    for (int i = 0; i < MX6_PIECES; ++i) __builtin_amdgcn_global_load_lds((gptr_t)(xg[i] + k0), (lptr_t)(base + i * 4096), 16, 0, 0);
  };
  const int wn = wave & 1, wm = wave >> 1;
  const int fj = lane & 15, fc = lane >> 4;
  // the wave's channel groups: group g covers channels 16 gi[g] .. + 15 = row groups (quads) 4 gi[g] .. + 3 of the companion.  Groups past N / 16 (the
  // last workgroup of a ragged N) read the last group and are masked at the store.  Row group q holds 96 B bytes (B = K / 32 blocks per row):
  // plane A [4 rows][B][16 B], plane B [4 rows][B][8 B] behind its 64 B bytes; its scale dwords are [B][4 rows]
  const int64_t B = K >> 5;
  const int ngrp = N >> 4;
  const unsigned char* W = reinterpret_cast<const unsigned char*>(a.w);
  const unsigned char* S = reinterpret_cast<const unsigned char*>(a.wscale);
  const unsigned char* W2 = reinterpret_cast<const unsigned char*>(a.w2);
  const unsigned char* S2 = reinterpret_cast<const unsigned char*>(a.w2scale);
  const int64_t la = (int64_t)(fj >> 2) * 96 * B + ((int64_t)(fj & 3) * B + fc) * 16;                  // the lane's block of slab 0 in plane A, from its group's start
  const int64_t lb = (int64_t)(fj >> 2) * 96 * B + 64 * B + ((int64_t)(fj & 3) * B + fc) * 8;          // ... in plane B
  const int64_t ls = ((int64_t)(fj >> 2) * B + fc) * 4;                                                // ... its scale dword
  const unsigned esh = 8 * (fj & 3);                                                                   // the lane's row inside the dword
  auto wload = [&](Mx6W& w, const unsigned char* cp, const unsigned char* ep, int t) {
#pragma unroll
    for (int g = 0; g < MX6_CG; ++g) {
      const int64_t gi = min(n0 / 16 + wn * MX6_CG + g, ngrp - 1);           // wave-uniform
      w.a[g] = *reinterpret_cast<const u32x4*>(cp + gi * 384 * B + la + (int64_t)t * 64);
      w.b[g] = *reinterpret_cast<const u32x2*>(cp + gi * 384 * B + lb + (int64_t)t * 32);
      w.e[g] = *reinterpret_cast<const unsigned*>(ep + gi * 16 * B + ls + (int64_t)t * 16);
    }
  };
  // row tiles of this wave that hold a row of the call (wave-uniform): the others are neither read from LDS nor multiplied
  const int nrt = __builtin_amdgcn_readfirstlane(max(0, min(MX6_RT, (M - m0 - wm * 32 + 15) / 16)));
  const int brow = (wm * 32 + fj) * 256;                                     // byte offset of the lane's row in tile 0; tile 1: + 16 rows
  f32x4 acc[MX6_CG][MX6_RT], acc2[DUAL ? MX6_CG : 1][DUAL ? MX6_RT : 1];
#pragma unroll
  for (int g = 0; g < MX6_CG; ++g)
#pragma unroll
    for (int r = 0; r < MX6_RT; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[g][r][e] = 0.f; if (DUAL) acc2[g][r][e] = 0.f; }

  // one slab against the wave's NRT live row tiles (a compile-time count: no branch around a load or an MFMA).  The lane's B fragments of the
  // slab are read once - MFMA h meets k = 32 c + 8 h + i, the row's piece 4 c + h - and each meets every channel group
  Mx6W cw, cw2, nw, nw2;
  auto slab = [&](auto NRT, const unsigned char* xs) {
    constexpr int R = decltype(NRT)::value;
    u32x4 fb[4][R];
#pragma unroll
    for (int h = 0; h < 4; ++h)
#pragma unroll
      for (int r = 0; r < R; ++r) fb[h][r] = *reinterpret_cast<const u32x4*>(xs + brow + r * 16 * 256 + (((4 * fc + h) ^ fj) << 4));
#pragma unroll
    for (int g = 0; g < MX6_CG; ++g) {
      const bf16x32 d = mx6_block(cw.a[g], cw.b[g], (cw.e[g] >> esh) & 0xffu);
      bf16x32 d2;
      if (DUAL) d2 = mx6_block(cw2.a[g], cw2.b[g], (cw2.e[g] >> esh) & 0xffu);
      bf16x8 fa[4], fa2[4];
      fa[0] = __builtin_shufflevector(d, d, 0, 1, 2, 3, 4, 5, 6, 7);
      fa[1] = __builtin_shufflevector(d, d, 8, 9, 10, 11, 12, 13, 14, 15);
      fa[2] = __builtin_shufflevector(d, d, 16, 17, 18, 19, 20, 21, 22, 23);
      fa[3] = __builtin_shufflevector(d, d, 24, 25, 26, 27, 28, 29, 30, 31);
      if (DUAL) {
        fa2[0] = __builtin_shufflevector(d2, d2, 0, 1, 2, 3, 4, 5, 6, 7);
        fa2[1] = __builtin_shufflevector(d2, d2, 8, 9, 10, 11, 12, 13, 14, 15);
        fa2[2] = __builtin_shufflevector(d2, d2, 16, 17, 18, 19, 20, 21, 22, 23);
        fa2[3] = __builtin_shufflevector(d2, d2, 24, 25, 26, 27, 28, 29, 30, 31);
      }
#pragma unroll
      for (int h = 0; h < 4; ++h)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          acc[g][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[h], __builtin_bit_cast(bf16x8, fb[h][r]), acc[g][r], 0, 0, 0);
          if (DUAL) acc2[g][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa2[h], __builtin_bit_cast(bf16x8, fb[h][r]), acc2[g][r], 0, 0, 0);
        }
    }
  };
  const int nk = K / MX6_BK;
  stage(0, 0);
  wload(cw, W, S, 0);
  if (DUAL) wload(cw2, W2, S2, 0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMAs (and codes) of slab t have landed
    __syncthreads();                                      // ... every wave's; and slab t - 1 is read out everywhere
    if (t + 1 < nk) {
      stage((t + 1) & 1, (t + 1) * MX6_BK);
      wload(nw, W, S, t + 1);
      if (DUAL) wload(nw2, W2, S2, t + 1);
    }
    const unsigned char* xs = xsm + (t & 1) * MX6_SLAB;
    if (nrt == MX6_RT) slab(std::integral_constant<int, MX6_RT>{}, xs);       // wave-uniform: one branch per slab, none inside it
    else if (nrt == 1) slab(std::integral_constant<int, 1>{}, xs);
    if (t + 1 < nk) { cw = nw; if (DUAL) cw2 = nw2; }
  }

  // epilogue: register e of group g is D[channel 4 (lane / 16) + e of the group][row lane % 16].
  // vv_gemm_mx6_check guarantees the 16-byte alignment of every vector access below
#pragma unroll
  for (int g = 0; g < MX6_CG; ++g) {
    const int n = n0 + (wn * MX6_CG + g) * 16 + 4 * fc;
    if (n >= N) continue;
#pragma unroll
    for (int r = 0; r < MX6_RT; ++r) {
      const int m = m0 + wm * 32 + r * 16 + fj;
      if (r >= nrt || m >= M) continue;
      float v[4] = {acc[g][r][0], acc[g][r][1], acc[g][r][2], acc[g][r][3]};
      if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
      if (DUAL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = vv_silu(v[i]) * acc2[g][r][i];
      }
      if (a.res) {
        const float4 rs = *reinterpret_cast<const float4*>(a.res + (int64_t)m * a.ldres + n);
        v[0] += rs.x; v[1] += rs.y; v[2] += rs.z; v[3] += rs.w;
      }
      if (OBF) {
        uint2 p;
        p.x = pack2(v[0], v[1]);
        p.y = pack2(v[2], v[3]);
        *reinterpret_cast<uint2*>(reinterpret_cast<bf16_t*>(a.out) + (int64_t)m * a.ldo + n) = p;
      } else {
        *reinterpret_cast<float4*>(a.out + (int64_t)m * a.ldo + n) = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  }
}

// every instantiation, once: the launch switch and the route name below read it and nothing else names them
#define VV_GEMM_MX6_FORMS(X) X(false, false) X(false, true) X(true, false) X(true, true)

long mx6_grid(const vv_lin_args& a) { return (long)((a.n + MX6_TN - 1) / MX6_TN) * ((a.m + MX6_TM - 1) / MX6_TM); }

}  // namespace

// The one place that says what a VV_LIN_W_MX6GEMM call must look like (linear_check_args asks it for vv_linear and vv_linear_route before anything
// is launched): host only, reads the arguments' values, follows no pointer.  0 = the kernel takes the call, else VV_E_UNSUPPORTED with the reason
int vv_gemm_mx6_check(const vv_lin_args& a) {
  const char* why = nullptr;
  if (a.wdt != VV_MXFP6) why = "wdt must be VV_MXFP6 (the companion layout)";
  else if (a.flags & VV_LIN_W_MXGEMM) why = "VV_LIN_W_MXGEMM names the GEMM on MXFP4 codes";
  else if (!(a.flags & VV_LIN_X_BF16)) why = "the activations must be bf16 (VV_LIN_X_BF16)";
  else if (a.flags & VV_LIN_W_FRAG) why = "VV_LIN_W_FRAG names another layout";
  else if (a.pro != VV_PRO_NONE || a.mod_scale) why = "no prologue on bf16 activations";
  else if (a.m < 3) why = "m >= 3 (1..2 rows stream the companion without the flag)";
  else if (a.n % 16) why = "n % 16 == 0";
  else if (a.k % MX6_BK) why = "k % 128 == 0";
  else if (!a.wscale || (a.w2 && !a.w2scale)) why = "the scale bytes are missing";
  else if (a.gate) why = "no gate epilogue";
  else if (a.w2 ? a.act != VV_ACT_SWIGLU : a.act != VV_ACT_NONE) why = "epilogues: bias, residual, SwiGLU pair";
  else if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16)) why = "the codes must be 16-byte aligned";
  else if ((uintptr_t)a.wscale % 4 || (a.w2 && (uintptr_t)a.w2scale % 4)) why = "the scale bytes must be 4-byte aligned";
  else if ((uintptr_t)a.x % 16 || a.ldx % 8) why = "x must be 16-byte aligned with ldx % 8 == 0";
  else if ((uintptr_t)a.out % 16 || a.ldo % 4 || (a.bias && (uintptr_t)a.bias % 16) || (a.res && ((uintptr_t)a.res % 16 || a.ldres % 4)))
    why = "out, bias and res must be 16-byte aligned with ldo % 4 == 0 and ldres % 4 == 0";
  else if (mx6_grid(a) > 0x7fffffffL) why = "too many tiles for one launch";
  if (!why) return 0;
  return vv_set_error(VV_E_UNSUPPORTED, "vv_linear: VV_LIN_W_MX6GEMM (the matrix-core GEMM on MXFP6 codes) not covered: %s (m=%d n=%d k=%d wdt=%d flags=%d)", why,
                      a.m, a.n, a.k, a.wdt, a.flags);
}

int vv_launch_gemm_mx6(const vv_lin_args& a, hipStream_t s) {
  const bool dual = a.w2 != nullptr, obf = (a.flags & VV_LIN_OUT_BF16) != 0;
#define X(D, O) if (dual == D && obf == O) hipLaunchKernelGGL((gemm_mx6_kernel<D, O>), dim3((unsigned)mx6_grid(a)), dim3(256), 0, s, a);
  VV_GEMM_MX6_FORMS(X)
#undef X
  return 0;
}

// the instantiation's name as the route query reports it: spelled here and nowhere else; a form the X-macro does not list has no name
int vv_gemm_mx6_route_name(const vv_lin_args& a, char* name, int cap) {
  const bool dual = a.w2 != nullptr, obf = (a.flags & VV_LIN_OUT_BF16) != 0;
#define X(D, O) if (dual == D && obf == O) return snprintf(name, (size_t)cap, "gemm_mx6<dual=%d,obf=%d>", (int)D, (int)O);
  VV_GEMM_MX6_FORMS(X)
#undef X
  name[0] = 0;
  return 0;
}

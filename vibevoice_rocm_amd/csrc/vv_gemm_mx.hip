// vv_gemm_mx.hip — the matrix-core GEMM on MXFP4 CODES: the prompt prefill and every other non-decode pass of 3 or more rows of a lean
// weight_quant="mxfp4" model (no bf16 copy of the matrix exists), reached through VV_LIN_W_MXGEMM with wdt == VV_MXFP4 only.
//   out[m, n] = epilogue(sum_k W_eff[n, k] * x[m, k])        m >= 3, n % 16 == 0, k % 128 == 0, x bf16 (VV_LIN_X_BF16, no prologue)
//   W_eff[n, k] = value(code) * 2^(e - 127), W in the VV_MXFP4 companion layout (pack_mxfp4, include/vv_hip.h): exact in bf16
// The weights never pass through LDS, a lookup table or memory in decoded form.  The companion's 16-byte piece is 4 rows x 8 k of one row QUAD, so
// lane 16 c + j of a wave loads the piece of quad j at k chunk c of a 32-wide k step (a wave load is 16 segments of 64 bytes) and the dword beside it
// that holds the four rows' E8M0 bytes of that 32-k block; dword t under byte t decodes (v_cvt_scalef32_pk_bf16_fp4, as mx_frag of
// vv_gemv_rows.hip) to the A fragment of MFMA t, whose 16 fragment rows are the weight rows 4 j + t, j = 0 .. 15.  Four MFMAs per load cover 64
// weight rows x 32 k; in the accumulators a lane then holds, for one activation row, the 16 CONSECUTIVE channels 16 (lane / 16) + 4 r + t
// (register r of MFMA t): the epilogue is four float4 per row tile with no shuffle.
// A workgroup owns 64 rows x 128 channels: 4 waves sit 2 (channels) x 2 (rows), each with 2 row tiles of 16.  The activations go global -> LDS by
// LDS-DMA as in vv_gemm_packed.hip (128-k slabs, two buffers, the bank swizzle on the source address: slot s of row r holds k piece s ^ (r & 15));
// the codes of slab t + 1 are requested into registers while the matrix cores work on slab t.
// Determinism: no atomics, no split K - every output element is one fp32 accumulator that meets the 32-wide k steps in ascending order, each
// step an MFMA whose result for one element depends on that element's weight row and activation row alone.  A row's result therefore does not
// depend on m, on the row's place in the call or on the other rows (tests/test_hip_gemm_mx.py holds this bit for bit).
// Measured alternatives and timings: profiles/mxfp4_lean.txt.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

constexpr int MX_TM = 64;                        // rows of a workgroup's tile
constexpr int MX_TN = 128;                       // channels of a workgroup's tile: 2 waves x 16 quads x 4 rows
constexpr int MX_BK = 128;                       // K elements per slab: a row is 256 bytes = 16 pieces of 16, four 32-wide MFMA steps
constexpr int MX_STEPS = MX_BK / 32;
constexpr int MX_SLAB = MX_TM * MX_BK * 2;       // bytes of one activation slab (16 KB)
constexpr int MX_PIECES = MX_SLAB / (16 * 256);  // DMA instructions per thread per slab (4)
constexpr int MX_RT = 2;                         // 16-row tiles per wave

// one slab's codes and scale dwords of one matrix, as a lane holds them
struct MxW { u32x4 c[MX_STEPS]; unsigned e[MX_STEPS]; };

template <bool DUAL, bool OBF>
__global__ __launch_bounds__(256) void gemm_mx_kernel(const vv_lin_args a) {
  __shared__ __attribute__((aligned(16))) unsigned char xsm[2 * MX_SLAB];     // [2 buffers][64 rows][16 slots of 16 bytes]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.m, K = a.k, N = a.n;
  const int mtiles = (M + MX_TM - 1) / MX_TM;
  const int wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int n0 = (wg / mtiles) * MX_TN, m0 = (wg % mtiles) * MX_TM;          // consecutive workgroups share the weight panel
  // piece p = 256 i + tid of a slab: LDS row p >> 4, slot p & 15 <- the row's k piece (p & 15) ^ (row & 15)
  const bf16_t* xg[MX_PIECES];
#pragma unroll
  for (int i = 0; i < MX_PIECES; ++i) {
    const int p = 256 * i + tid, row = p >> 4, kp = (p & 15) ^ (row & 15);
    xg[i] = reinterpret_cast<const bf16_t*>(a.x) + (int64_t)min(m0 + row, M - 1) * a.ldx + kp * 8;       // rows past M: a valid row, masked at the store
  }
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto stage = [&](int buf, int k0) {
    unsigned char* base = xsm + buf * MX_SLAB + wave * 1024;                 // wave-uniform: the DMA adds lane * 16
#pragma unroll
    for (int i = 0; i < MX_PIECES; ++i) __builtin_amdgcn_global_load_lds((gptr_t)(xg[i] + k0), (lptr_t)(base + i * 4096), 16, 0, 0);
  };
  const int wn = wave & 1, wm = wave >> 1;
  const int fj = lane & 15, fc = lane >> 4;
  // the lane's quad: rows 4 q .. 4 q + 3.  Quads past N / 4 (the last workgroup of a ragged N) read the last quad and are masked at the store
  const int ku = (K + 511) >> 9;
  const int q = min(n0 / 4 + wn * 16 + fj, N / 4 - 1);
  // piece (k0 / 8 + 4 step + c) of the quad's row of pieces: units of 512 k are 64 pieces, blocks of 32 k are 4 - no unit arithmetic is left
  const u32x4* wp = reinterpret_cast<const u32x4*>(a.w) + (int64_t)q * ku * 64 + fc;
  const unsigned* sp = reinterpret_cast<const unsigned*>(a.wscale) + (int64_t)q * ku * 16;
  const u32x4* wp2 = DUAL ? reinterpret_cast<const u32x4*>(a.w2) + (int64_t)q * ku * 64 + fc : nullptr;
  const unsigned* sp2 = DUAL ? reinterpret_cast<const unsigned*>(a.w2scale) + (int64_t)q * ku * 16 : nullptr;
  auto wload = [&](MxW& w, const u32x4* cp, const unsigned* ep, int k0) {
#pragma unroll
    for (int s = 0; s < MX_STEPS; ++s) { w.c[s] = cp[(k0 >> 3) + 4 * s]; w.e[s] = ep[(k0 >> 5) + s]; }
  };
  // row tiles of this wave that hold a row of the call (wave-uniform): the others are neither read from LDS nor multiplied
  const int nrt = __builtin_amdgcn_readfirstlane(max(0, min(MX_RT, (M - m0 - wm * 32 + 15) / 16)));
  const int brow = (wm * 32 + fj) * 256;                                     // byte offset of the lane's row in tile 0; tile 1: + 16 rows
  f32x4 acc[4][MX_RT], acc2[DUAL ? 4 : 1][DUAL ? MX_RT : 1];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < MX_RT; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[t][r][e] = 0.f; if (DUAL) acc2[t][r][e] = 0.f; }

  const int nk = K / MX_BK;
  MxW cw, cw2, nw, nw2;
  stage(0, 0);
  wload(cw, wp, sp, 0);
  if (DUAL) wload(cw2, wp2, sp2, 0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMAs (and codes) of slab t have landed
    __syncthreads();                                      // ... every wave's; and slab t - 1 is read out everywhere
    if (t + 1 < nk) {
      stage((t + 1) & 1, (t + 1) * MX_BK);
      wload(nw, wp, sp, (t + 1) * MX_BK);
      if (DUAL) wload(nw2, wp2, sp2, (t + 1) * MX_BK);
    }
    const unsigned char* xs = xsm + (t & 1) * MX_SLAB;
#pragma unroll
    for (int s = 0; s < MX_STEPS; ++s) {
      u32x4 fb[MX_RT];
#pragma unroll
      for (int r = 0; r < MX_RT; ++r)
        if (r < nrt) fb[r] = *reinterpret_cast<const u32x4*>(xs + brow + r * 16 * 256 + (((4 * s + fc) ^ fj) << 4));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 fa = mx_frag(cw.c[s][i], (cw.e[s] >> (8 * i)) & 0xffu);
        bf16x8 fa2;
        if (DUAL) fa2 = mx_frag(cw2.c[s][i], (cw2.e[s] >> (8 * i)) & 0xffu);
#pragma unroll
        for (int r = 0; r < MX_RT; ++r)
          if (r < nrt) {
            acc[i][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, __builtin_bit_cast(bf16x8, fb[r]), acc[i][r], 0, 0, 0);
            if (DUAL) acc2[i][r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa2, __builtin_bit_cast(bf16x8, fb[r]), acc2[i][r], 0, 0, 0);
          }
      }
    }
    if (t + 1 < nk) { cw = nw; if (DUAL) cw2 = nw2; }
  }

  // epilogue: register e of MFMA i is D[quad 4 (lane / 16) + e][row lane % 16] = channel 16 (lane / 16) + 4 e + i of the wave's 64.
  // vv_gemm_mx_check guarantees the 16-byte alignment of every vector access below
  const int nb = n0 + wn * 64 + 16 * fc;
  if (nb >= N) return;
#pragma unroll
  for (int r = 0; r < MX_RT; ++r) {
    const int m = m0 + wm * 32 + r * 16 + fj;
    if (r >= nrt || m >= M) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = nb + 4 * e;
      float v[4] = {acc[0][r][e], acc[1][r][e], acc[2][r][e], acc[3][r][e]};
      if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
      if (DUAL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = vv_silu(v[i]) * acc2[i][r][e];
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

// every instantiation, once: the launch switch below and nothing else names them
#define VV_GEMM_MX_FORMS(X) X(false, false) X(false, true) X(true, false) X(true, true)

long mx_grid(const vv_lin_args& a) { return (long)((a.n + MX_TN - 1) / MX_TN) * ((a.m + MX_TM - 1) / MX_TM); }

}  // namespace

// The one place that says what a VV_LIN_W_MXGEMM call must look like (vv_linear and vv_linear_route ask it before anything is launched): host
// only, reads the arguments' values, follows no pointer.  0 = the kernel takes the call, else VV_E_UNSUPPORTED with the reason
int vv_gemm_mx_check(const vv_lin_args& a) {
  const char* why = nullptr;
  if (a.wdt != VV_MXFP4) why = "wdt must be VV_MXFP4 (the companion layout)";
  else if (!(a.flags & VV_LIN_X_BF16)) why = "the activations must be bf16 (VV_LIN_X_BF16)";
  else if (a.flags & VV_LIN_W_FRAG) why = "VV_LIN_W_FRAG names another layout";
  else if (a.pro != VV_PRO_NONE || a.mod_scale) why = "no prologue on bf16 activations";
  else if (a.m < 3) why = "m >= 3 (1..2 rows stream the companion without the flag)";
  else if (a.n % 16) why = "n % 16 == 0";
  else if (a.k % MX_BK) why = "k % 128 == 0";
  else if (!a.wscale || (a.w2 && !a.w2scale)) why = "the scale bytes are missing";
  else if (a.gate) why = "no gate epilogue";
  else if (a.w2 ? a.act != VV_ACT_SWIGLU : a.act != VV_ACT_NONE) why = "epilogues: bias, residual, SwiGLU pair";
  else if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16) || (uintptr_t)a.wscale % 16 || (a.w2 && (uintptr_t)a.w2scale % 16)) why = "codes and scale bytes must be 16-byte aligned";
  else if ((uintptr_t)a.x % 16 || a.ldx % 8) why = "x must be 16-byte aligned with ldx % 8 == 0";
  else if ((uintptr_t)a.out % 16 || a.ldo % 4 || (a.bias && (uintptr_t)a.bias % 16) || (a.res && ((uintptr_t)a.res % 16 || a.ldres % 4)))
    why = "out, bias and res must be 16-byte aligned with ldo % 4 == 0 and ldres % 4 == 0";
  else if (mx_grid(a) > 0x7fffffffL) why = "too many tiles for one launch";
  if (!why) return 0;
  return vv_set_error(VV_E_UNSUPPORTED, "vv_linear: VV_LIN_W_MXGEMM (the matrix-core GEMM on MXFP4 codes) not covered: %s (m=%d n=%d k=%d flags=%d)", why, a.m,
                      a.n, a.k, a.flags);
}

int vv_launch_gemm_mx(const vv_lin_args& a, hipStream_t s) {
  const bool dual = a.w2 != nullptr, obf = (a.flags & VV_LIN_OUT_BF16) != 0;
#define X(D, O) if (dual == D && obf == O) hipLaunchKernelGGL((gemm_mx_kernel<D, O>), dim3((unsigned)mx_grid(a)), dim3(256), 0, s, a);
  VV_GEMM_MX_FORMS(X)
#undef X
  return 0;
}

// the instantiation's name as the route query reports it: spelled here and nowhere else
int vv_gemm_mx_route_name(const vv_lin_args& a, char* name, int cap) {
  return snprintf(name, (size_t)cap, "gemm_mx<dual=%d,obf=%d>", a.w2 != nullptr, (a.flags & VV_LIN_OUT_BF16) != 0);
}

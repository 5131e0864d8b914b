// vv_gemm_packed.hip — the prompt prefill's GEMMs at PACKED row counts (several dialogues' prompts in one pass: 700 .. 4 000 rows of bf16
// activations against the bf16 LLM matrices), reached through VV_LIN_PACKED only.
//   out[m, n] = epilogue(sum_k W[n, k] * x[m, k])          n % 128 == 0, k % 64 == 0, x bf16 (VV_LIN_X_BF16, no prologue)
// A workgroup owns a 128 x 128 output tile; the K loop walks 64-deep slabs.  Both operands go global -> LDS by LDS-DMA
// (global_load_lds, 16 bytes per lane): no staging registers, no ds_write pass.  The DMA's LDS destination is wave-uniform base + lane * 16,
// so the LDS image is lane-linear - piece p = 256 i + tid of a slab lies at byte 16 p, row p / 8, slot p % 8 - and the bank swizzle sits on the
// SOURCE address: slot s of row r holds the row's 16-byte k piece s ^ ((r >> 1) & 7).  A fragment read (32 rows, one k piece) then spreads every
// 16 consecutive rows over the 16 slots of the 256-byte bank row.  Two LDS buffers: slab t + 1 is in flight while the matrix cores work on slab t.
// Per K step: wait for the own DMAs of slab t (vmcnt(0)), barrier, issue slab t + 1 into the other buffer, multiply slab t.  The barrier orders
// both hazards: every wave's DMAs of slab t have landed before any wave reads it (the read follows the barrier that follows the wait), and
// every wave has finished reading slab t - 1 before its buffer is written again.
// 4 waves sit 2 x 2, each with 2 x 2 (dual: twice that) mfma_f32_32x32x16_bf16 accumulators.  All LDS is one array.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

constexpr int PK_T = 128;                        // tile rows of every operand (and of the output, both ways)
constexpr int PK_BK = 64;                        // K elements per slab: a row is 128 bytes = 8 pieces of 16
constexpr int PK_SLAB = PK_T * PK_BK * 2;        // bytes of one operand slab (16 KB)
constexpr int PK_PIECES = PK_SLAB / (16 * 256);  // DMA instructions per thread per operand slab (4)

// Measured on the MI355X against the routes these calls take without the flag (tools/mb_packed_prefill.py, profiles/packed_prefill.txt): of
// M = 128, 330, 712, 1 320, 2 640, 4 096 rows, 2 640 is the smallest from which this kernel is faster on every 1.5B and 7B prefill matrix
// (1.15x .. 1.74x; at 1 320 rows the 1.5B o and down projections still lose 0.76x / 0.73x to the 64 x 64 tiles, which fill more of the chip)
constexpr int PK_ROWS_DEFAULT = 2640;
int g_packed_rows = PK_ROWS_DEFAULT;             // fewest rows for this kernel (tuning hook "gemm_packed_rows"; 0 = never, < 0 = back to the default)

template <bool DUAL, bool OBF>
__global__ __launch_bounds__(256) void gemm_packed_kernel(const vv_lin_args a) {
  constexpr int NOP = DUAL ? 3 : 2;              // operand slabs per buffer: x, w (, w2)
  extern __shared__ __attribute__((aligned(16))) unsigned char psm[];     // [2 buffers][NOP][PK_SLAB]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = a.m, K = a.k;
  const int mtiles = (M + PK_T - 1) / PK_T;
  const int wg = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const int n0 = (wg / mtiles) * PK_T, m0 = (wg % mtiles) * PK_T;        // consecutive workgroups share the weight panel
  // piece p = 256 i + tid: LDS row p >> 3, slot p & 7 <- the row's k piece (p & 7) ^ ((row >> 1) & 7)
  const bf16_t* xg[PK_PIECES]; const bf16_t* wg1[PK_PIECES]; const bf16_t* wg2[PK_PIECES];
#pragma unroll
  for (int i = 0; i < PK_PIECES; ++i) {
    const int p = 256 * i + tid, row = p >> 3, kp = (p & 7) ^ ((row >> 1) & 7);
    xg[i] = reinterpret_cast<const bf16_t*>(a.x) + (int64_t)min(m0 + row, M - 1) * a.ldx + kp * 8;     // rows past M: a valid row, masked at the store
    wg1[i] = reinterpret_cast<const bf16_t*>(a.w) + (int64_t)(n0 + row) * K + kp * 8;
    wg2[i] = DUAL ? reinterpret_cast<const bf16_t*>(a.w2) + (int64_t)(n0 + row) * K + kp * 8 : nullptr;
  }
  typedef const __attribute__((address_space(1))) void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  auto stage = [&](int buf, int k0) {
    unsigned char* base = psm + buf * (NOP * PK_SLAB) + wave * 1024;       // wave-uniform: the DMA adds lane * 16
#pragma unroll
    for (int i = 0; i < PK_PIECES; ++i) {
      __builtin_amdgcn_global_load_lds((gptr_t)(xg[i] + k0), (lptr_t)(base + i * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(wg1[i] + k0), (lptr_t)(base + PK_SLAB + i * 4096), 16, 0, 0);
      if (DUAL) __builtin_amdgcn_global_load_lds((gptr_t)(wg2[i] + k0), (lptr_t)(base + 2 * PK_SLAB + i * 4096), 16, 0, 0);
    }
  };
  const int wn = wave & 1, wm = wave >> 1;
  const int fr = lane & 31, fh = lane >> 5;
  // byte offset of this lane's fragment row inside a slab, and the row's swizzle
  int arow[2], asw[2], brow[2], bsw[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int ra = wn * 64 + i * 32 + fr, rb = wm * 64 + i * 32 + fr;
    arow[i] = ra * 128; asw[i] = (ra >> 1) & 7;
    brow[i] = rb * 128; bsw[i] = (rb >> 1) & 7;
  }
  f32x16 acc[2][2], acc2[DUAL ? 2 : 1][DUAL ? 2 : 1];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[i][j][r] = 0.f; if (DUAL) acc2[i][j][r] = 0.f; }

  const int nk = K / PK_BK;
  stage(0, 0);
  for (int t = 0; t < nk; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMAs of slab t have landed
    __syncthreads();                                      // ... every wave's; and slab t - 1 is read out everywhere
    if (t + 1 < nk) stage((t + 1) & 1, (t + 1) * PK_BK);
    const unsigned char* xs = psm + (t & 1) * (NOP * PK_SLAB);
    const unsigned char* ws1 = xs + PK_SLAB;
    const unsigned char* ws2 = xs + 2 * PK_SLAB;
#pragma unroll
    for (int sub = 0; sub < PK_BK / 16; ++sub) {
      const int kp = sub * 2 + fh;
      u32x4 fa[2], fb[2], fa2[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = *reinterpret_cast<const u32x4*>(ws1 + arow[i] + ((kp ^ asw[i]) << 4));
        if (DUAL) fa2[i] = *reinterpret_cast<const u32x4*>(ws2 + arow[i] + ((kp ^ asw[i]) << 4));
        fb[i] = *reinterpret_cast<const u32x4*>(xs + brow[i] + ((kp ^ bsw[i]) << 4));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa[i]), __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0);
          if (DUAL) acc2[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fa2[i]), __builtin_bit_cast(bf16x8, fb[j]), acc2[i][j], 0, 0, 0);
        }
    }
  }

  // epilogue: D[n = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)][m = lane & 31] - a lane holds 4 runs of 4 consecutive channels of one row.
  // packed_covers guarantees the 16-byte alignment of every vector access below
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + wm * 64 + j * 32 + fr;
      if (m >= M) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 64 + i * 32 + 8 * g + 4 * fh;
        float v[4] = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
        if (a.bias) { const float4 b = *reinterpret_cast<const float4*>(a.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
        if (DUAL) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = vv_silu(v[e]) * acc2[i][j][4 * g + e];
        }
        if (a.res) {
          const float4 r = *reinterpret_cast<const float4*>(a.res + (int64_t)m * a.ldres + n);
          v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
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

template <bool DUAL> constexpr int packed_lds() { return 2 * (DUAL ? 3 : 2) * PK_SLAB; }

template <bool DUAL, bool OBF>
void launch_packed(const vv_lin_args& a, hipStream_t s) {
  const int nwg = (a.n / PK_T) * ((a.m + PK_T - 1) / PK_T);
  hipLaunchKernelGGL((gemm_packed_kernel<DUAL, OBF>), dim3(nwg), dim3(256), packed_lds<DUAL>(), s, a);
}

}  // namespace

// The one place that decides whether a vv_linear call runs here: VV_LIN_PACKED, enough rows, and the shapes / alignments the kernel's DMA
// and vector epilogue need.  Host only: reads the arguments' values, follows no pointer.  Anything else routes as if the flag were not set.
bool vv_gemm_packed_covers(const vv_lin_args& a) {
  if (!(a.flags & VV_LIN_PACKED) || g_packed_rows <= 0 || a.m < g_packed_rows) return false;
  if (a.wdt != VV_BF16 || !(a.flags & VV_LIN_X_BF16) || (a.flags & VV_LIN_W_FRAG) || a.pro != VV_PRO_NONE) return false;
  if (a.n % PK_T || a.k % PK_BK || a.ldx % 8 || a.gate || a.mod_scale) return false;
  if (a.w2 ? a.act != VV_ACT_SWIGLU : a.act != VV_ACT_NONE) return false;
  if ((long)(a.n / PK_T) * ((a.m + PK_T - 1) / PK_T) > 0x7fffffffL) return false;
  if ((uintptr_t)a.x % 16 || (uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16) || (uintptr_t)a.out % 16 || a.ldo % 4) return false;
  if ((a.bias && (uintptr_t)a.bias % 16) || (a.res && ((uintptr_t)a.res % 16 || a.ldres % 4))) return false;
  return true;
}

int vv_launch_gemm_packed(const vv_lin_args& a, hipStream_t s) {
  const bool obf = (a.flags & VV_LIN_OUT_BF16) != 0;
  if (a.w2) { if (obf) launch_packed<true, true>(a, s); else launch_packed<true, false>(a, s); }
  else { if (obf) launch_packed<false, true>(a, s); else launch_packed<false, false>(a, s); }
  return 0;
}

// the instantiation's name as the route query reports it
int vv_gemm_packed_route_name(const vv_lin_args& a, char* name, int cap) {
  return snprintf(name, (size_t)cap, "gemm_packed<dual=%d,obf=%d>", a.w2 != nullptr, (a.flags & VV_LIN_OUT_BF16) != 0);
}

void vv_gemm_packed_set_rows(int rows) { g_packed_rows = rows < 0 ? PK_ROWS_DEFAULT : rows; }

// graph capture must not see the one-time hipFuncSetAttribute calls: vv_init warms them here
int vv_gemm_packed_init() {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_packed_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, packed_lds<false>()) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_packed_kernel<false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, packed_lds<false>()) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_packed_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize, packed_lds<true>()) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_packed_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, packed_lds<true>()) != hipSuccess)
    return vv_set_error(VV_E_HIP, "gemm_packed init: cannot raise the LDS limit");
  return 0;
}

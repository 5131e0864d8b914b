// vv_conv_hot.hip — shape-specialised kernels for the conv tokenizers' one-row stage (C = 2048, one row per frame) and the two GEMVs that
// hand a frame over between that stage and the C = 1024 stage (bf16 weights, fp32 rows, M = 1).  The pattern is vv_gemv_hot.hip's: N, K,
// the K split and the rows per block are compile-time constants, only the call site's epilogue exists, there is no row loop, and a wave
// requests ALL the weights it owns at kernel entry behind the few operand loads it needs first.
//
// The arithmetic of every output element is that of the path it replaces, so the results are bit-identical (tests/test_hip_conv_hot.py
// compares with torch.equal):
//   conv_gemv   the generic gemv_stream_kernel<1, false, NW, KU, 2>: 512-element K units interleaved over the block's NW waves, packed-FMA
//               order inside a unit and over units, vv_wave_sum, combine over waves 0 .. NW - 1 from 0.f, then + bias, (* gate, + res) as a
//               product and a sum
//   row_in      ffn_in_row_kernel (vv_convffn.hip): the same statistics, the same bf16 image, mfma_f32_32x32x16_bf16 over a K quarter per
//               wave in 32 steps of 16, the four-wave sum in wave order, + b1, vv_gelu_as
//
//   entry              call site (vv_model.hip)                              n x k          grid x waves   per block
//   block.w2           second FFN GEMV of a one-row Block1D                  2048 x 8192    256 x 4        8 rows (bit 8: 512 x 4, 4 rows)
//   block.ffn_in_row   mixer + RMSNorm + W1 + GELU of a one-row Block1D      8192 x 2048    256 + 1 x 4    32 hidden channels; + 1: the history shift
//   dec.handover       decoder's transposed conv 2048 -> 8 x 1024           8192 x 4096    1024 x 4       8 rows (bit 8: 512 x 4, 16 rows)
//   sem.handover       encoder's stride-8 conv 16 x 1024 -> 2048             2048 x 16384   512 x 8        4 rows (bit 8: 256 x 8, 8 rows)
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "vv_hip.h"
#include "vv_common.h"

namespace {

typedef unsigned short bf16_t;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void unpack8(const u32x4 v, float (&o)[8]) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
}

template <bool NT>
__device__ __forceinline__ u32x4 ldw(const bf16_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

// one lane's 8 weights of one K unit against the activation row: even / odd k accumulate separately (v_pk_fma_f32), j ascending
__device__ __forceinline__ void fma_unit(const u32x4 wv, const float (&x)[8], vf2& p) {
  float w[8];
  unpack8(wv, w);
#pragma unroll
  for (int j = 0; j < 8; j += 2) p = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, vf2{x[j], x[j + 1]}, p);
}

// v * gate + res as the generic epilogue rounds it: a product and a sum, never one FMA
__device__ __forceinline__ float gate_res(float v, float g, float r) {
#pragma clang fp contract(off)
  const float t = v * g;
  return t + r;
}

#define VV_FENCE4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))

// ---------------------------------------------------------------------------------------------------------------------------------
// M = 1 GEMV, K split over the block's NW waves in interleaved 512-element units (wave w: units w, w + NW, ...), R consecutive output
// rows per block, one combine through LDS.  GR: epilogue (+ bias) * gate[n] + res[n] (the one-row block's W2); else + bias.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int N, int K, int NW, int R, bool GR>
__global__ __launch_bounds__(64 * NW) void conv_gemv_kernel(const vv_lin_args a) {
  constexpr int KU = K / (512 * NW);
  static_assert(K % (512 * NW) == 0 && N % R == 0 && R <= 64 && R * KU + 2 * KU + 3 < 63, "whole units, whole row sets, every load in flight at once");
  __shared__ float part[NW][R];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = (int)blockIdx.x * R;
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);

  int koff[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) koff[u] = (wave + NW * u) * 512 + lane * 8;
  float4 xa[KU], xb[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    xa[u] = *reinterpret_cast<const float4*>(a.x + koff[u]);
    xb[u] = *reinterpret_cast<const float4*>(a.x + koff[u] + 4);
  }
  // epilogue operands of output r in thread r; the other threads fetch output 0's: no divergent branch around the loads
  const int eo_n = n0 + (tid < R ? tid : 0);
  const float eb = a.bias[eo_n];
  float eg = 1.f, er = 0.f;
  if constexpr (GR) { eg = a.gate[eo_n]; er = a.res[eo_n]; }
  u32x4 wq[R][KU];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int u = 0; u < KU; ++u) wq[r][u] = ldw<true>(W + (n0 + r) * K + koff[u]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < KU; ++u) { VV_FENCE4(xa[u]); VV_FENCE4(xb[u]); }

  float xr[KU][8];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    xr[u][0] = xa[u].x; xr[u][1] = xa[u].y; xr[u][2] = xa[u].z; xr[u][3] = xa[u].w;
    xr[u][4] = xb[u].x; xr[u][5] = xb[u].y; xr[u][6] = xb[u].z; xr[u][7] = xb[u].w;
  }
  float acc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    vf2 p = vf2{0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KU; ++u) fma_unit(wq[r][u], xr[u], p);
    acc[r] = vv_wave_sum(p.x + p.y);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) part[wave][r] = acc[r];
  }
  __syncthreads();
  if (tid < R) {
    float s = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < NW; ++w4) s += part[w4][tid];
    float v = s + eb;
    if constexpr (GR) v = gate_res(v, eg, er);
    a.out[eo_n] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The first FFN half of a one-row Block1D: ffn_in_row_kernel's arithmetic with
//   * the history shift on a workgroup of its own (block 256: x, norm_w and five history rows, no weights) instead of 40 more registers and
//     ten more loads in front of workgroup 0's weights, on the launch's critical path;
//   * the four-wave combine, + b1 and GELU in 32 threads, one hidden channel each (one 128-byte store), instead of 8 threads with four
//     channels each, and only the tile's one real activation column through LDS;
//   * NT (tuning bit 9, off): W1 requested with non-temporal loads like the GEMVs' weights.  Measured 2.4 us SLOWER per launch.  A likely
//     reason, not verified with counters: a lane's 16 bytes of MFMA steps s .. s + 3 share a 128-byte line, and only cacheable loads let the
//     four requests meet in the vector cache.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int pack2(float a, float b) {
  const __hip_bfloat16 x = __float2bfloat16(a), y = __float2bfloat16(b);
  return (unsigned int)(*reinterpret_cast<const bf16_t*>(&x)) | ((unsigned int)(*reinterpret_cast<const bf16_t*>(&y)) << 16);
}
__device__ __forceinline__ void ld4(const float* p, float (&o)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

constexpr int ROW_C = 2048, ROW_WG = 4 * ROW_C / 32;    // 256 workgroups of 32 hidden channels; workgroup ROW_WG shifts the history

template <bool NT>
__global__ __launch_bounds__(256) void row_in_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ hidden,
                                                     float* __restrict__ hist_new, const vv_block B, float eps) {
  constexpr int C = ROW_C, P1 = C + 8, ST = C / 64;
  __shared__ __attribute__((aligned(16))) bf16_t xh[P1];
  __shared__ float red[4 * 16 * 2];
  __shared__ float part[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int c0[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) c0[j] = 4 * (tid + 256 * j);

  if (blockIdx.x == ROW_WG) {                      // the keeper: history rows 1..5 move up, the normalised new row goes last
    float xv[2][4], nw[2][4], hrow[5][2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ld4(x + c0[j], xv[j]);
      ld4(B.norm_w + c0[j], nw[j]);
    }
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int j = 0; j < 2; ++j) ld4(B.hist + (size_t)(r + 1) * C + c0[j], hrow[r][j]);
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) q = fmaf(xv[j][e], xv[j][e], q);
    q = vv_wave_sum(q);
    if (lane == 0) part[wave] = q;
    __syncthreads();
    const float rstd1 = rsqrtf(((part[0] + part[1]) + (part[2] + part[3])) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float xn[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) xn[e] = xv[j][e] * rstd1 * nw[j][e];
#pragma unroll
      for (int r = 0; r < 5; ++r) st4(hist_new + (size_t)r * C + c0[j], hrow[r][j]);
      st4(hist_new + (size_t)5 * C + c0[j], xn);
    }
    return;
  }

  const int n0 = blockIdx.x * 32;
  const int lm = lane & 31, hk = (lane >> 5) * 8;
  float xv[2][4], hsv[2][4], dl[2][4], nw[2][4], db[2][4], gm[2][4], fw[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    ld4(x + c0[j], xv[j]);
    ld4(B.norm_w + c0[j], nw[j]);
    ld4(B.hs + c0[j], hsv[j]);
    ld4(B.dw_last + c0[j], dl[j]);
    ld4(B.dw_b + c0[j], db[j]);
    ld4(B.gamma + c0[j], gm[j]);
    ld4(B.ffn_norm_w + c0[j], fw[j]);
  }
  u32x4 wf[ST];
  {
    const bf16_t* wr = reinterpret_cast<const bf16_t*>(B.w1) + (int64_t)(n0 + lm) * C + wave * (C / 4) + hk;
#pragma unroll
    for (int s = 0; s < ST; ++s) wf[s] = ldw<NT>(wr + s * 16);
  }
  const float b1v = B.b1[n0 + lm];                 // thread o < 32 finishes hidden channel n0 + o
  __builtin_amdgcn_sched_barrier(0);
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) q = fmaf(xv[j][e], xv[j][e], q);
  q = vv_wave_sum(q);
  if (lane == 0) part[wave] = q;
  __syncthreads();
  const float rstd1 = rsqrtf(((part[0] + part[1]) + (part[2] + part[3])) / (float)C + eps);
  float yv[2][4], xn[2][4];
  float q2 = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      xn[j][e] = xv[j][e] * rstd1 * nw[j][e];
      const float sc = db[j][e] + hsv[j][e] + dl[j][e] * xn[j][e];
      yv[j][e] = xv[j][e] + gm[j][e] * sc;
      q2 = fmaf(yv[j][e], yv[j][e], q2);
    }
  q2 = vv_wave_sum(q2);
  if (lane == 0) part[4 + wave] = q2;
  __syncthreads();
  const float rstd2 = rsqrtf(((part[4] + part[5]) + (part[6] + part[7])) / (float)C + eps);
  {
    const int ys0 = blockIdx.x * (C / ROW_WG);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      uint2 p;
      p.x = pack2(yv[j][0] * rstd2 * fw[j][0], yv[j][1] * rstd2 * fw[j][1]);
      p.y = pack2(yv[j][2] * rstd2 * fw[j][2], yv[j][3] * rstd2 * fw[j][3]);
      *reinterpret_cast<uint2*>(xh + c0[j]) = p;
      if (c0[j] >= ys0 && c0[j] < ys0 + C / ROW_WG) st4(y + c0[j], yv[j]);
    }
  }
  __syncthreads();
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  {
    const bf16_t* xf = xh + wave * (C / 4) + hk;                   // every tile column reads the one row
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      const u32x4 xb = *reinterpret_cast<const u32x4*>(xf + s * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[s]), __builtin_bit_cast(bf16x8, xb), acc, 0, 0, 0);
    }
  }
  // tile column 0 sits in lanes 0 and 32: register r of lane 32 h is channel 8 (r / 4) + 4 h + r % 4
  if (lm == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[(wave * 16 + r) * 2 + (lane >> 5)] = acc[r];
  }
  __syncthreads();
  if (tid < 32) {
    const int r = 4 * (tid >> 3) + (tid & 3), h = (tid >> 2) & 1;
    float s = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) s += red[(w4 * 16 + r) * 2 + h];
    hidden[n0 + tid] = vv_gelu_as(s + b1v);
  }
}

#undef VV_FENCE4

// table order == bit order of the "conv_hot" tuning key
constexpr int N_HOT = 4;
const vv_conv_hot_shape g_table[N_HOT] = {
    // name               kind              m  n     k      bias gate res
    {"block.w2",         VV_CONV_HOT_GEMV, 1, 2048, 8192,  1,   1,   1},
    {"block.ffn_in_row", VV_CONV_HOT_ROW,  1, 8192, 2048,  1,   0,   0},
    {"dec.handover",     VV_CONV_HOT_GEMV, 1, 8192, 4096,  1,   0,   0},
    {"sem.handover",     VV_CONV_HOT_GEMV, 1, 2048, 16384, 1,   0,   0},
};

constexpr int HOT_DEFAULT = 0xf;   // the adopted entries (tools/mb_conv_hot.py)
// tuning hook "conv_hot": bit i = table entry i takes its hot kernel; bit 8 = the GEMVs on their other measured rows-per-block choice (see the
// table at the top); bit 9 = W1 of ffn_in_row with non-temporal instead of cacheable loads
int g_hot = HOT_DEFAULT;

bool matches(const vv_conv_hot_shape& e, const vv_lin_args& a) {
  return e.kind == VV_CONV_HOT_GEMV && a.m == e.m && a.n == e.n && a.k == e.k && a.wdt == VV_BF16 && !a.w2 && a.pro == VV_PRO_NONE && !a.mod_scale &&
         !a.mod_shift && (a.bias != nullptr) == (e.bias != 0) && (a.gate != nullptr) == (e.gate != 0) && (!e.gate || a.gate_ld == 0) &&
         (a.res != nullptr) == (e.res != 0) && a.act == VV_ACT_NONE && a.flags == 0;
}

}  // namespace

void vv_conv_hot_set(int mask) { g_hot = mask < 0 ? HOT_DEFAULT : mask; }   // negative: back to the adopted set

extern "C" int vv_conv_hot_shapes(vv_conv_hot_shape* out, int cap) {
  for (int i = 0; i < N_HOT && i < cap; ++i) out[i] = g_table[i];
  return N_HOT;
}

// The decision: index of the enabled GEMV table entry the call equals, or -1 (the caller goes on to the generic template).  No launch, no pointer followed.
int vv_conv_hot_gemv_covers(const vv_lin_args& a) {
  if (!(g_hot & ((1 << N_HOT) - 1)) || a.m != 1 || a.wdt != VV_BF16) return -1;
  for (int i = 0; i < N_HOT; ++i)
    if ((g_hot >> i & 1) && matches(g_table[i], a)) return i;
  return -1;
}

// The launch of table entry id (from vv_conv_hot_gemv_covers): 1 = launched.  The caller has checked the 16-byte alignment of x and w.
int vv_launch_conv_hot_gemv(const vv_lin_args& a, int id, hipStream_t s) {
  const bool alt = (g_hot & 256) != 0;
  switch (id) {
    case 0:
      if (alt) hipLaunchKernelGGL((conv_gemv_kernel<2048, 8192, 4, 4, true>), dim3(512), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((conv_gemv_kernel<2048, 8192, 4, 8, true>), dim3(256), dim3(256), 0, s, a);
      return 1;
    case 2:
      if (alt) hipLaunchKernelGGL((conv_gemv_kernel<8192, 4096, 4, 16, false>), dim3(512), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((conv_gemv_kernel<8192, 4096, 4, 8, false>), dim3(1024), dim3(256), 0, s, a);
      return 1;
    case 3:
      if (alt) hipLaunchKernelGGL((conv_gemv_kernel<2048, 16384, 8, 8, false>), dim3(256), dim3(512), 0, s, a);
      else hipLaunchKernelGGL((conv_gemv_kernel<2048, 16384, 8, 4, false>), dim3(512), dim3(512), 0, s, a);
      return 1;
  }
  return 0;
}

// 1 = launched, 0 = entry switched off.  The caller (vv_launch_ffn_in_row_hs) has checked bf16 weights, C, the pointers and their alignment.
int vv_launch_conv_hot_row(const vv_block& B, const float* x, float* y, float* hidden, float* hist_new, int C, float eps, hipStream_t s) {
  if (!(g_hot & 2) || C != ROW_C || !hist_new) return 0;
  if (!(g_hot & 512)) hipLaunchKernelGGL(row_in_kernel<false>, dim3(ROW_WG + 1), dim3(256), 0, s, x, y, hidden, hist_new, B, eps);
  else hipLaunchKernelGGL(row_in_kernel<true>, dim3(ROW_WG + 1), dim3(256), 0, s, x, y, hidden, hist_new, B, eps);
  return 1;
}

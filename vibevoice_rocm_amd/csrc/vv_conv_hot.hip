// vv_conv_hot.hip — shape-specialised kernels for the conv tokenizers' one-row stage (C = 2048, one row per frame and dialogue) and the two GEMVs
// that hand a frame over between that stage and the C = 1024 stage (bf16 weights, fp32 rows), for ONE dialogue (the default path) and for the
// B = 2..8 dialogues of a row batch in one pass over the weights (vv_decoder_front_rows / vv_encoder_back_rows, vv_model.hip).  The pattern
// is vv_gemv_hot.hip's: N, K, the K split and the rows per block are compile-time constants, only the call site's epilogue exists, and a wave
// requests ALL the weights it owns at kernel entry.  The row-in kernel is one template with the row count BT as its first argument: the one-row
// kernel is its BT == 1 instance, so row b of a batch equals it bit for bit by construction.  The GEMV is two kernels with one arithmetic
// (see rows_gemv_kernel for why).
//
// The arithmetic of every output element is that of the path it replaces, so the results are bit-identical (tests/test_hip_conv_hot.py
// compares with torch.equal):
//   conv_gemv   the generic gemv_stream_kernel<1, false, NW, KU, 2>: 512-element K units interleaved over the block's NW waves, packed-FMA
//               order inside a unit and over units, vv_wave_sum, combine over waves 0 .. NW - 1 from 0.f, then + bias, (* gate, + res) as a
//               product and a sum
//   rows_gemv   conv_gemv for BT activation rows: the weights a wave owns are requested once and used for every row; per (output, row) the
//               K units, the packed-FMA order, the wave sum and the combine over the waves are conv_gemv_kernel's, so row b equals the
//               one-row GEMV bit for bit.  No split-K across blocks: deterministic.
//   row_in_rows ffn_in_row_kernel (vv_convffn.hip): the same statistics, the same bf16 image, mfma_f32_32x32x16_bf16 over a K quarter per
//               wave in 32 steps of 16, the four-wave sum in wave order, + b1, vv_gelu_as.  BT rows: the mixer and both RMSNorms run per
//               row, row b goes into tile column b - columns that the one-row instance computes from the one row and throws away.
//   rows_ctx    masked state movement of a row batch: gather (state -> padded conv inputs, the net's input rides along) and scatter (scratch
//               histories -> hist with hs refreshed, conv left contexts, output rows) - stores of a scatter reach ACTIVE dialogues only.
// Every dialogue of a row batch keeps its own streaming state: the B nets are forks of one net, so dialogue b's state lives at dialogue 0's
// address + delta[b] floats (vv_rows_delta).
//
//   entry              call site (vv_model.hip)                              n x k          grid x waves   per block
//   block.w2           second FFN GEMV of a one-row Block1D                  2048 x 8192    256 x 4        8 rows (bit 8: 512 x 4, 4 rows)
//   block.ffn_in_row   mixer + RMSNorm + W1 + GELU of a one-row Block1D      8192 x 2048    256 + 1 x 4    32 hidden channels; + 1: the history shift
//   dec.handover       decoder's transposed conv 2048 -> 8 x 1024           8192 x 4096    1024 x 4       8 rows (bit 8: 512 x 4, 16 rows)
//   sem.handover       encoder's stride-8 conv 16 x 1024 -> 2048             2048 x 16384   512 x 8        4 rows (bit 8: 256 x 8, 8 rows)
// A row batch takes w2 on 512 x 4 (4 rows per block) and the hand-overs on their default grids.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

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
// out[b, n] = epilogue(sum_k W[n, k] x[b, k]) for BT rows; K split over the block's NW waves in interleaved 512-element units, R output channels per
// block, one combine through LDS.  GR: (+ bias) * gate[n] + res[b, n]; else + bias.  active (or NULL): rows of dialogues with active == 0 are not stored.
// Not conv_gemv_kernel's BT == 1 instance: that kernel walks its weights output by output, the order it requested them in, with its one row's
// K units resident; this one walks them unit by unit so that a pass holds one unit of each row, and stores every wave sum at once.  Its BT == 1
// instance was measured on the MI355X at + 0.33 .. 0.62 us per W2 launch and + 0.2 .. 0.35 us per hand-over against conv_gemv_kernel, with the
// weights requested unit by unit as well as output by output (profiles/conv_fold.txt); the one-row order at BT > 1 keeps BT x KU x 8 more registers.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int BT, int N, int K, int NW, int R, bool GR, int HB>
__global__ __launch_bounds__(64 * NW) void rows_gemv_kernel(const float* __restrict__ x, int64_t ldx, const bf16_t* __restrict__ W,
                                                            const float* __restrict__ bias, const float* __restrict__ gate, const float* res,
                                                            int64_t ldres, float* out, int64_t ldo, const int* __restrict__ active) {
  constexpr int KU = K / (512 * NW);
  static_assert(K % (512 * NW) == 0 && N % R == 0 && R * BT <= 64 * NW, "whole units, whole channel sets, one epilogue thread per output");
  __shared__ float part[NW][R * BT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = (int)blockIdx.x * R;
  int koff[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) koff[u] = (wave + NW * u) * 512 + lane * 8;
  // epilogue operands of output (r, b) in thread r * BT + b; the other threads fetch output (0, 0)'s: no divergent branch around the loads
  const int et = tid < R * BT ? tid : 0;
  const int er_ = et / BT, eb_ = et - er_ * BT;
  const float ebias = bias[n0 + er_];
  float eg = 1.f, er = 0.f;
  if constexpr (GR) { eg = gate[n0 + er_]; er = res[(int64_t)eb_ * ldres + n0 + er_]; }
  const int eact = active ? active[eb_] : 1;
  u32x4 wq[R][KU];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int u = 0; u < KU; ++u) wq[r][u] = ldw<true>(W + (int64_t)(n0 + r) * K + koff[u]);
  __builtin_amdgcn_sched_barrier(0);

  // HB rows per pass over the (register-resident) weights: 8 waves share 512 registers per lane, and the scheduler keeps the activation rows
  // of every K unit of a pass in flight - BT x KU x 8 registers would spill from 6 rows on
#pragma unroll
  for (int b0 = 0; b0 < BT; b0 += HB) {
    vf2 p[R][HB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) p[r][bb] = vf2{0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) {
        if (b0 + bb >= BT) continue;                 // (compile time)
        const float* xp = x + (int64_t)(b0 + bb) * ldx + koff[u];
        const float4 xa = *reinterpret_cast<const float4*>(xp);
        const float4 xb = *reinterpret_cast<const float4*>(xp + 4);
        const float xr[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
        for (int r = 0; r < R; ++r) fma_unit(wq[r][u], xr, p[r][bb]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int bb = 0; bb < HB; ++bb) {
        if (b0 + bb >= BT) continue;
        const float a = vv_wave_sum(p[r][bb].x + p[r][bb].y);
        if (lane == 0) part[wave][r * BT + b0 + bb] = a;
      }
    __builtin_amdgcn_sched_barrier(0);               // the next pass's loads stay behind this pass
  }
  __syncthreads();
  if (tid < R * BT) {
    float s = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < NW; ++w4) s += part[w4][tid];
    float v = s + ebias;
    if constexpr (GR) v = gate_res(v, eg, er);
    if (eact) out[(int64_t)eb_ * ldo + n0 + er_] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The first FFN half of a one-row Block1D for BT rows: ffn_in_row_kernel's arithmetic with
//   * the history shift on workgroups of their own (block 256 + b: x, norm_w and five history rows of dialogue b, no weights) instead of 40
//     more registers and ten more loads in front of workgroup 0's weights, on the launch's critical path;
//   * the four-wave combine, + b1 and GELU in 32 threads per row, one hidden channel each (one 128-byte store), instead of 8 threads with four
//     channels each, and only the tile's BT real activation columns through LDS;
//   * NT (tuning bit 9, off; BT == 1 only): W1 requested with non-temporal loads like the GEMVs' weights.  Measured 2.4 us SLOWER per launch
//     (DESIGN.md 5e).  A likely reason, not verified with counters: a lane's 16 bytes of MFMA steps s .. s + 3 share a 128-byte line, and only
//     cacheable loads let the four requests meet in the vector cache.
// x[BT, C], y[BT, C], hidden[BT, 4C], hist_new[BT][6, C] (BT > 1: scratch); B: dialogue 0's block.  BT > 1: hs / hist of dialogue b at + dl.d[b],
// the histories of active dialogues only; BT == 1 reads neither dl nor active.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int ROW_C = 2048, ROW_WG = 4 * ROW_C / 32;    // 256 workgroups of 32 hidden channels; workgroup ROW_WG + b shifts dialogue b's history

template <int BT, bool NT>
__global__ __launch_bounds__(256) void row_in_rows_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ hidden,
                                                          float* __restrict__ hist_new, const vv_block B, float eps, const vv_rows_delta dl,
                                                          const int* __restrict__ active) {
  constexpr int C = ROW_C, P1 = C + 8, ST = C / 64;
  static_assert(BT == 1 || !NT, "the non-temporal W1 variant exists for one row only");
  __shared__ __attribute__((aligned(16))) bf16_t xh[BT * P1];
  __shared__ float red[4 * 16 * 2 * BT];
  __shared__ float part[BT * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int c0[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) c0[j] = 4 * (tid + 256 * j);

  if (blockIdx.x >= ROW_WG) {                      // a keeper: dialogue b's history rows 1..5 move up, the normalised new row goes last
    const int b = BT == 1 ? 0 : blockIdx.x - ROW_WG;
    const float* hist = B.hist;
    if constexpr (BT > 1) {
      if (!active[b]) return;                      // (uniform over the workgroup)
      hist += dl.d[b];
    }
    const float* xr = x + (size_t)b * C;
    float* hn = hist_new + (size_t)b * 6 * C;
    float xv[2][4], nw[2][4], hrow[5][2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ld4(xr + c0[j], xv[j]);
      ld4(B.norm_w + c0[j], nw[j]);
    }
#pragma unroll
    for (int r = 0; r < 5; ++r)
#pragma unroll
      for (int j = 0; j < 2; ++j) ld4(hist + (size_t)(r + 1) * C + c0[j], hrow[r][j]);
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
      for (int r = 0; r < 5; ++r) st4(hn + (size_t)r * C + c0[j], hrow[r][j]);
      st4(hn + (size_t)5 * C + c0[j], xn);
    }
    return;
  }

  const int n0 = blockIdx.x * 32;
  const int lm = lane & 31, hk = (lane >> 5) * 8;
  float xv[BT][2][4], hsv[BT][2][4];
  float dwl[2][4], nw[2][4], db[2][4], gm[2][4], fw[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int b = 0; b < BT; ++b) ld4(x + (size_t)b * C + c0[j], xv[b][j]);
    ld4(B.norm_w + c0[j], nw[j]);
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      const float* hs = B.hs;
      if constexpr (BT > 1) hs += dl.d[b];
      ld4(hs + c0[j], hsv[b][j]);
    }
    ld4(B.dw_last + c0[j], dwl[j]);
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
  const float b1v = B.b1[n0 + lm];                 // thread 32 b + o finishes hidden channel n0 + o of row b
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int b = 0; b < BT; ++b) {
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) q = fmaf(xv[b][j][e], xv[b][j][e], q);
    q = vv_wave_sum(q);
    if (lane == 0) part[b * 8 + wave] = q;
  }
  __syncthreads();
#pragma unroll
  for (int b = 0; b < BT; ++b) {                   // xv becomes y, in place
    const float* pb = part + b * 8;
    const float rstd1 = rsqrtf(((pb[0] + pb[1]) + (pb[2] + pb[3])) / (float)C + eps);
    float q2 = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float xn = xv[b][j][e] * rstd1 * nw[j][e];
        const float sc = db[j][e] + hsv[b][j][e] + dwl[j][e] * xn;
        xv[b][j][e] = xv[b][j][e] + gm[j][e] * sc;
        q2 = fmaf(xv[b][j][e], xv[b][j][e], q2);
      }
    q2 = vv_wave_sum(q2);
    if (lane == 0) part[b * 8 + 4 + wave] = q2;
  }
  __syncthreads();
  {
    const int ys0 = blockIdx.x * (C / ROW_WG);
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      const float* pb = part + b * 8 + 4;
      const float rstd2 = rsqrtf(((pb[0] + pb[1]) + (pb[2] + pb[3])) / (float)C + eps);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint2 p;
        p.x = pack2(xv[b][j][0] * rstd2 * fw[j][0], xv[b][j][1] * rstd2 * fw[j][1]);
        p.y = pack2(xv[b][j][2] * rstd2 * fw[j][2], xv[b][j][3] * rstd2 * fw[j][3]);
        *reinterpret_cast<uint2*>(xh + b * P1 + c0[j]) = p;
        if (c0[j] >= ys0 && c0[j] < ys0 + C / ROW_WG) st4(y + (size_t)b * C + c0[j], xv[b][j]);
      }
    }
  }
  __syncthreads();
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  {
    const bf16_t* xf = xh + min(lm, BT - 1) * P1 + wave * (C / 4) + hk;      // tile column b reads row b; columns past BT repeat the last row (never stored)
#pragma unroll
    for (int s = 0; s < ST; ++s) {
      const u32x4 xb = *reinterpret_cast<const u32x4*>(xf + s * 16);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[s]), __builtin_bit_cast(bf16x8, xb), acc, 0, 0, 0);
    }
  }
  // tile column b sits in lanes b and 32 + b: register r of lane 32 h + b is channel 8 (r / 4) + 4 h + r % 4 of row b
  if (lm < BT) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wave * 16 + r) * 2 + (lane >> 5)) * BT + lm] = acc[r];
  }
  __syncthreads();
  if (tid < 32 * BT) {
    const int b = tid >> 5, o = tid & 31;
    const int r = 4 * (o >> 3) + (o & 3), h = (o >> 2) & 1;
    float s = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) s += red[((w4 * 16 + r) * 2 + h) * BT + b];      // wave order: the same sum for every BT
    hidden[(size_t)b * 4 * C + n0 + o] = vv_gelu_as(s + b1v);
  }
}

struct CtxRowsArgs { vv_rows_item it[VV_ROWS_ITEMS]; vv_rows_delta dl; int n; };

// grid (chunks, items, B).  gather: buf_b <- other_b (every dialogue: only the workspace is written); scatter: other_b <- buf_b for ACTIVE dialogues,
// and for a block history hs_b[c] = sum_k<6 dw_w[c, k] * buf_b[k, c] (the one-row composites' closing scatter, bit for bit)
__global__ __launch_bounds__(256) void rows_ctx_kernel(const CtxRowsArgs a, const int* __restrict__ active, int scatter) {
  const vv_rows_item it = a.it[blockIdx.y];
  const int b = blockIdx.z;
  if (scatter && !active[b]) return;
  float* buf = it.buf + (int64_t)b * it.ld_buf;
  float* oth = it.other + (it.relocate ? a.dl.d[b] : (int64_t)b * it.ld_other);
  const int n = it.n;
  if (!scatter) {
    if (it.affine) {
      for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) buf[i] = fmaf(oth[i], it.scale, it.bias);
      return;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) buf[i] = oth[i];
    return;
  }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) oth[i] = buf[i];
  if (it.hs) {
    float* hs = it.hs + a.dl.d[b];
    for (int c = blockIdx.x * 256 + threadIdx.x; c < it.C; c += gridDim.x * 256) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) s = fmaf(it.dw_w[(size_t)c * 7 + k], buf[(size_t)k * it.C + c], s);
      hs[c] = s;
    }
  }
}

// out[b * rows_out + r, :] = src[b, :] for r < rows_out, active dialogues only
__global__ __launch_bounds__(256) void rows_bcast_kernel(const float* __restrict__ src, int64_t ld_src, float* __restrict__ out, int64_t ldo, int rows_out, int n,
                                                         const int* __restrict__ active) {
  const int b = blockIdx.y;
  if (active && !active[b]) return;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const float v = src[(int64_t)b * ld_src + i];
    for (int r = 0; r < rows_out; ++r) out[((int64_t)b * rows_out + r) * ldo + i] = v;
  }
}

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

bool a16(const void* q) { return q && ((uintptr_t)q % 16) == 0; }

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
  const vv_rows_delta none{};                      // the one-row instance reads neither of the two
  const int* active = nullptr;
  if (!(g_hot & 512)) hipLaunchKernelGGL((row_in_rows_kernel<1, false>), dim3(ROW_WG + 1), dim3(256), 0, s, x, y, hidden, hist_new, B, eps, none, active);
  else hipLaunchKernelGGL((row_in_rows_kernel<1, true>), dim3(ROW_WG + 1), dim3(256), 0, s, x, y, hidden, hist_new, B, eps, none, active);
  return 1;
}

// 0 = enqueued.  The caller (vv_model.hip) has checked C = 2048, bf16 weights, 2 <= nb <= 8 and that B.hs / hist / dw_last exist
int vv_launch_row_in_rows(const vv_block& B, int nb, const float* x, float* y, float* hidden, float* hist_new, const vv_rows_delta& dl, const int* active,
                          float eps, hipStream_t s) {
  if (!a16(B.w1) || !a16(B.b1) || !a16(B.gamma) || !a16(B.norm_w) || !a16(B.ffn_norm_w) || !a16(B.dw_b) || !a16(B.dw_last) || !a16(B.hs) || !a16(B.hist) ||
      !a16(x) || !a16(y) || !a16(hidden) || !a16(hist_new) || !active || x == y)
    return vv_set_error(VV_E_ARG, "vv_conv_rows: misaligned or missing operand of the one-row block");
  for (int b = 0; b < nb; ++b)
    if (dl.d[b] % 4) return vv_set_error(VV_E_ARG, "vv_conv_rows: dialogue %d's state is not 16-byte aligned to dialogue 0's", b);
#define VV_RIR(BT) case BT: hipLaunchKernelGGL((row_in_rows_kernel<BT, false>), dim3(ROW_WG + BT), dim3(256), 0, s, x, y, hidden, hist_new, B, eps, dl, active); break
  switch (nb) {
    VV_RIR(2); VV_RIR(3); VV_RIR(4); VV_RIR(5); VV_RIR(6); VV_RIR(7); VV_RIR(8);
    default: return vv_set_error(VV_E_UNSUPPORTED, "vv_conv_rows: %d rows (2..8)", nb);
  }
#undef VV_RIR
  VV_CHECK_LAUNCH("row_in_rows");
  return 0;
}

// shape: VV_ROWS_W2 (2048 x 8192, * gate + res), VV_ROWS_DEC (8192 x 4096), VV_ROWS_SEM (2048 x 16384); 0 = enqueued
int vv_launch_rows_gemv(int shape, int nb, const float* x, int64_t ldx, const void* w, const float* bias, const float* gate, const float* res,
                        int64_t ldres, float* out, int64_t ldo, const int* active, hipStream_t s) {
  if (!a16(x) || !a16(w) || !bias || !out || ldx % 4 || (shape == VV_ROWS_W2 && (!gate || !res)))
    return vv_set_error(VV_E_ARG, "vv_conv_rows: misaligned or missing operand of a %d-row GEMV", nb);
  const bf16_t* W = reinterpret_cast<const bf16_t*>(w);
#define VV_RG(BT, N, K, NW, R, GR, HB) \
  hipLaunchKernelGGL((rows_gemv_kernel<BT, N, K, NW, R, GR, HB>), dim3(N / R), dim3(64 * NW), 0, s, x, ldx, W, bias, gate, res, ldres, out, ldo, active)
#define VV_RGS(BT)                                                      \
  case BT:                                                              \
    if (shape == VV_ROWS_W2) VV_RG(BT, 2048, 8192, 4, 4, true, BT);     \
    else if (shape == VV_ROWS_DEC) VV_RG(BT, 8192, 4096, 4, 8, false, BT); \
    else VV_RG(BT, 2048, 16384, 8, 4, false, (BT >= 7 ? 2 : BT == 6 ? 3 : BT)); \
    break
  if (shape != VV_ROWS_W2 && shape != VV_ROWS_DEC && shape != VV_ROWS_SEM) return vv_set_error(VV_E_ARG, "vv_conv_rows: GEMV shape %d", shape);
  switch (nb) {
    VV_RGS(2); VV_RGS(3); VV_RGS(4); VV_RGS(5); VV_RGS(6); VV_RGS(7); VV_RGS(8);
    default: return vv_set_error(VV_E_UNSUPPORTED, "vv_conv_rows: %d rows (2..8)", nb);
  }
#undef VV_RGS
#undef VV_RG
  VV_CHECK_LAUNCH("rows_gemv");
  return 0;
}

int vv_launch_rows_ctx(const vv_rows_item* items, int n, int nb, const vv_rows_delta& dl, const int* active, int scatter, hipStream_t s) {
  if (n <= 0) return 0;
  if (n > VV_ROWS_ITEMS || nb < 1 || nb > 8 || (scatter && !active)) return vv_set_error(VV_E_ARG, "vv_conv_rows: state move list");
  CtxRowsArgs a;
  a.n = n; a.dl = dl;
  int mx = 0;
  for (int i = 0; i < n; ++i) { a.it[i] = items[i]; if (items[i].n > mx) mx = items[i].n; }
  for (int i = n; i < VV_ROWS_ITEMS; ++i) a.it[i] = vv_rows_item{};
  int bx = (mx + 1023) / 1024;
  if (bx > 16) bx = 16;
  if (bx < 1) bx = 1;
  hipLaunchKernelGGL(rows_ctx_kernel, dim3(bx, n, nb), dim3(256), 0, s, a, active, scatter);
  VV_CHECK_LAUNCH("rows_ctx");
  return 0;
}

int vv_launch_rows_bcast(const float* src, int64_t ld_src, float* out, int64_t ldo, int rows_out, int n, int nb, const int* active, hipStream_t s) {
  hipLaunchKernelGGL(rows_bcast_kernel, dim3((n + 255) / 256 < 16 ? (n + 255) / 256 : 16, nb), dim3(256), 0, s, src, ld_src, out, ldo, rows_out, n, active);
  VV_CHECK_LAUNCH("rows_bcast");
  return 0;
}

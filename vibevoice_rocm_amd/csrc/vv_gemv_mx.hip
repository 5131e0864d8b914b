// vv_gemv_mx.hip — the batch-1/2 weight-streaming GEMV on OCP MXFP4 weights (VV_MXFP4: e2m1 codes + one E8M0 scale byte per 32 k of a row).
//
// The memory side is that of vv_gemv_stream.hip: persistent waves, every weight byte read once with 16-byte (non-temporal unless
// VV_LIN_W_REUSED) loads straight into VGPRs, the first two row groups requested ahead of the activation prologue, the lane's fp32 activation
// slice in registers for the whole kernel, fp32 accumulation, DPP row sums, each output's epilogue in a lane of its own on operands fetched one
// row group ahead.  A row group is FOUR weight rows: a lane's 16-byte load carries the 32 codes of its own 8-wide k slice of one 512-wide unit
// in each of the 4 rows (layout: include/vv_hip.h), and one 4-byte load per unit carries the four rows' scale bytes of the lane's 32-block.
// Decode is the vector ALU's own: v_cvt_scalef32_pk_f32_fp4 turns one byte (two codes) and the block scale 2^(e - 127), built as
// __uint_as_float(e << 23), into two scaled fp32 weights - four per dword of codes, no table, no LDS.
//   KSPLIT == 1     a wave owns 4 whole weight rows per step (block = 4 independent waves)          K <= 2560 (SwiGLU: 2048)
//   KSPLIT == 4/8   the block's 4/8 waves split K (interleaved 512-element units) and combine through LDS in a fixed order
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float wsum(float v) { return vv_wave_sum(v); }   // DPP row reduction, all 64 lanes active
__device__ __forceinline__ float silu1(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float gelu1(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

// epilogue operands (bias / adaLN gate / residual) of one output, loaded one row group ahead (see vv_gemv_stream.hip: loads return in order)
struct EpiOp { float b, g, r; };
__device__ __forceinline__ EpiOp epi_load(const vv_lin_args& a, int m, int n) {
  // straight-line and use-free: an absent operand reads x[0] (always a valid address), the values are only looked at in epi_pre
  EpiOp e;
  const float* pb = a.bias ? a.bias + n : a.x;
  const float* pg = a.gate ? a.gate + (a.gate_ld ? (int64_t)m * a.gate_ld + n : (int64_t)n) : a.x;
  const float* pr = a.res ? a.res + (int64_t)m * a.ldres + n : a.x;
  e.b = *pb; e.g = *pg; e.r = *pr;
  return e;
}
__device__ __forceinline__ void epi_pre(const vv_lin_args& a, int m, int n, float v, float v2, const EpiOp& e) {
  if (a.bias) v += e.b;
  if (a.act == VV_ACT_GELU) v = gelu1(v);
  else if (a.act == VV_ACT_SWIGLU) v = silu1(v) * v2;
  if (a.gate) v *= e.g;
  if (a.res) v += e.r;
  a.out[(int64_t)m * a.ldo + n] = v;
}

// the 8 weights of one dword of codes (nibble i = k0 + i) under scale byte e: byte b of the dword holds k0 + 2 b (low nibble) and k0 + 2 b + 1
__device__ __forceinline__ void unpack8_mx(unsigned int c, unsigned int e, vf2 (&w)[4]) {
  const float s = __uint_as_float(e << 23);
  w[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 0);
  w[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 1);
  w[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 2);
  w[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 3);
}

int g_mx_blocks = 0;          // tuning hook "gemv_mx_blocks" (vv_tune): grid override, so that a test makes one wave walk many row groups
constexpr int RW = 4;         // weight rows per row group: one dword of codes each in a lane's 16-byte load

template <int M, bool DUAL, int KSPLIT, int KU>
__global__ __launch_bounds__(KSPLIT == 1 ? 512 : 64 * KSPLIT) void gemv_mx_kernel(const vv_lin_args a, const int n_groups) {
  constexpr int NW = (KSPLIT == 1) ? 8 : KSPLIT;     // waves per block (KSPLIT == 1: at most; the launcher starts 4)
  constexpr int ND = DUAL ? KU : 1;
  __shared__ float red[NW * M];
  __shared__ float part[2][NW][RW * M * 2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwv = (KSPLIT == 1) ? (int)(blockDim.x >> 6) : KSPLIT;
  const int K = a.k, N = a.n, mr = a.m;          // mr <= M real rows
  const unsigned char* __restrict__ C1 = reinterpret_cast<const unsigned char*>(a.w);
  const unsigned char* __restrict__ C2 = reinterpret_cast<const unsigned char*>(a.w2);
  const unsigned char* __restrict__ S1 = reinterpret_cast<const unsigned char*>(a.wscale);
  const unsigned char* __restrict__ S2 = reinterpret_cast<const unsigned char*>(a.w2scale);

  // ---- this lane's k offsets and activation fragment (kept in registers for the whole kernel) -------------------
  int koff[KU];
  bool kval[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int unit = (KSPLIT == 1) ? u : (wave + NW * u);
    koff[u] = unit * 512 + lane * 8;
    kval[u] = koff[u] < K;
    if (!kval[u]) koff[u] = 0;                    // any valid address; the activation there is forced to 0
  }
  const bool reused = (a.flags & VV_LIN_W_REUSED) != 0;
  const int units_k = (K + 511) >> 9;            // 512-wide units per row in the packed layout
  const int gstride = (KSPLIT == 1) ? gridDim.x * nwv : gridDim.x;
  int g = (KSPLIT == 1) ? blockIdx.x * nwv + wave : blockIdx.x;
  // one row group of one weight stream: KU x 16 bytes of codes (dword r = row r) and KU scale dwords (byte r = row r)
  u32x4 cur[KU], cur2[ND], nxt[KU], nxt2[ND];
  unsigned int sc[KU], sc2[ND], nsc[KU], nsc2[ND];
  auto issue = [&](u32x4 (&b)[KU], u32x4 (&b2)[ND], unsigned int (&s)[KU], unsigned int (&s2)[ND], int grp) {
    // a group past the end (the unconditional second issue of a wave that owns a single group) and a unit past the row's end read
    // offset 0 of the matrix: always inside it
    const bool live = grp < n_groups;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int unit = (KSPLIT == 1) ? u : (wave + NW * u);
      const bool ok = live && unit < units_k;
      const int64_t gu = ok ? (int64_t)grp * units_k + unit : 0;
      const int64_t co = ok ? (gu * 64 + lane) * 16 : 0;
      const int64_t so = ok ? (gu * 16 + (lane >> 2)) * 4 : 0;
      const u32x4* p1 = reinterpret_cast<const u32x4*>(C1 + co);
      const u32x4* p2 = reinterpret_cast<const u32x4*>(C2 + co);
      if (reused) { b[u] = *p1; if constexpr (DUAL) b2[u] = *p2; }
      else { b[u] = __builtin_nontemporal_load(p1); if constexpr (DUAL) b2[u] = __builtin_nontemporal_load(p2); }
      s[u] = *reinterpret_cast<const unsigned int*>(S1 + so);
      if constexpr (DUAL) s2[u] = *reinterpret_cast<const unsigned int*>(S2 + so);
    }
  };
  // epilogue: output (r, m) of a row group belongs to lane / thread  r * M + m  (KSPLIT == 1: lane of the wave that owns the
  // group; K split: thread of the block); each owner fetches its own operands one group ahead
  const bool has_eo = a.bias || a.gate || a.res;
  const int eid = (KSPLIT == 1) ? lane : tid;
  EpiOp eo_cur, eo_nxt;
  const int eo_id = eid < RW * M ? eid : 0;       // lanes that own no output fetch output 0's operands: no divergent branch around the loads
  const int eo_r = eo_id / M, eo_m = (eo_id - eo_r * M) < mr ? (eo_id - eo_r * M) : mr - 1;
  auto load_eo = [&](EpiOp& e, int grp) {
    if (!has_eo) return;
    e = epi_load(a, eo_m, min((grp < n_groups ? grp : n_groups - 1) * RW + eo_r, N - 1));
  };
  eo_cur.b = 0.f; eo_cur.g = 1.f; eo_cur.r = 0.f; eo_nxt = eo_cur;
  float xr[M][KU][8];
  // Activation side, as in vv_gemv_stream.hip.  BATCHED (M * KU <= 8, RMSNorm without adaLN rows or no prologue): every load the prologue
  // needs is issued in one batch AHEAD of the weight loads, which go out unconditionally behind it; the arithmetic runs while the first two
  // row groups of weights are in flight.  Everything else (SiLU, adaLN-modulated rows, long fragments) issues the weights first and walks
  // the rows unit by unit.
  constexpr bool BATCHED = M * KU <= 8;
  const bool batched = BATCHED && ((a.pro == VV_PRO_RMSNORM && !a.mod_scale) || a.pro == VV_PRO_NONE);
  if (BATCHED && batched) {
    float4 xa[M][KU], xb[M][KU], na[KU], nb[KU];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float* xrow = a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        xa[m][u] = *reinterpret_cast<const float4*>(xrow + koff[u]);
        xb[m][u] = *reinterpret_cast<const float4*>(xrow + koff[u] + 4);
      }
    }
    const bool rms = a.pro == VV_PRO_RMSNORM;
    const bool has_nw = rms && a.norm_w;
    if (has_nw) {
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        na[u] = *reinterpret_cast<const float4*>(a.norm_w + koff[u]);
        nb[u] = *reinterpret_cast<const float4*>(a.norm_w + koff[u] + 4);
      }
    }
    load_eo(eo_cur, g);
    issue(cur, cur2, sc, sc2, g);
    load_eo(eo_nxt, g + gstride);
    issue(nxt, nxt2, nsc, nsc2, g + gstride);
    __builtin_amdgcn_sched_barrier(0);
    // everything the prologue computes with is made opaque HERE, behind the weight loads, so that none of its arithmetic (and the waits it
    // needs) is hoisted in front of the weight issue
#define VV_FENCE4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int m = 0; m < M; ++m) { VV_FENCE4(xa[m][u]); VV_FENCE4(xb[m][u]); }
      if (has_nw) { VV_FENCE4(na[u]); VV_FENCE4(nb[u]); }
    }
#undef VV_FENCE4
    float ss[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      ss[m] = 0.f;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const bool kv = kval[u];                         // lanes past K read a valid address and contribute zeros
        xr[m][u][0] = kv ? xa[m][u].x : 0.f; xr[m][u][1] = kv ? xa[m][u].y : 0.f; xr[m][u][2] = kv ? xa[m][u].z : 0.f; xr[m][u][3] = kv ? xa[m][u].w : 0.f;
        xr[m][u][4] = kv ? xb[m][u].x : 0.f; xr[m][u][5] = kv ? xb[m][u].y : 0.f; xr[m][u][6] = kv ? xb[m][u].z : 0.f; xr[m][u][7] = kv ? xb[m][u].w : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) ss[m] = fmaf(xr[m][u][j], xr[m][u][j], ss[m]);
      }
    }
    if (rms) {
#pragma unroll
      for (int m = 0; m < M; ++m) ss[m] = wsum(ss[m]);   // KSPLIT == 1: every wave holds the whole row
      if (KSPLIT != 1) {
        if (lane == 0) {
#pragma unroll
          for (int m = 0; m < M; ++m) red[wave * M + m] = ss[m];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < M; ++m) {
          ss[m] = 0.f;
#pragma unroll
          for (int w4 = 0; w4 < nwv; ++w4) ss[m] += red[w4 * M + m];
        }
      }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float rstd = rsqrtf(ss[m] / (float)K + a.eps);
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          const float nw[8] = {na[u].x, na[u].y, na[u].z, na[u].w, nb[u].x, nb[u].y, nb[u].z, nb[u].w};
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = xr[m][u][j] * rstd;
            if (has_nw) v *= nw[j];
            xr[m][u][j] = kval[u] ? v : 0.f;
          }
        }
      }
    }
  } else {
    if (g < n_groups) { load_eo(eo_cur, g); issue(cur, cur2, sc, sc2, g); }
    if (g + gstride < n_groups) { load_eo(eo_nxt, g + gstride); issue(nxt, nxt2, nsc, nsc2, g + gstride); }   // two row groups in flight before the prologue starts
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float* xrow = a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx;
      float ss = 0.f;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if (kval[u]) {
          const float4 p = *reinterpret_cast<const float4*>(xrow + koff[u]);
          const float4 q = *reinterpret_cast<const float4*>(xrow + koff[u] + 4);
          xr[m][u][0] = p.x; xr[m][u][1] = p.y; xr[m][u][2] = p.z; xr[m][u][3] = p.w;
          xr[m][u][4] = q.x; xr[m][u][5] = q.y; xr[m][u][6] = q.z; xr[m][u][7] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xr[m][u][j] = 0.f;
        }
        if (a.pro == VV_PRO_SILU) {
#pragma unroll
          for (int j = 0; j < 8; ++j) xr[m][u][j] = silu1(xr[m][u][j]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) ss = fmaf(xr[m][u][j], xr[m][u][j], ss);
      }
      if (a.pro == VV_PRO_RMSNORM) {
        ss = wsum(ss);                               // KSPLIT == 1: every wave holds the whole row
        if (KSPLIT != 1) {
          if (lane == 0) red[wave * M + m] = ss;
          __syncthreads();
          ss = 0.f;
#pragma unroll
          for (int w4 = 0; w4 < nwv; ++w4) ss += red[w4 * M + m];
        }
        const float rstd = rsqrtf(ss / (float)K + a.eps);
#pragma unroll
        for (int u = 0; u < KU; ++u) {
          if (!kval[u]) continue;
          float nw[8], sh[8], sv[8];
          if (a.norm_w) {
            const float4 p = *reinterpret_cast<const float4*>(a.norm_w + koff[u]);
            const float4 q = *reinterpret_cast<const float4*>(a.norm_w + koff[u] + 4);
            nw[0] = p.x; nw[1] = p.y; nw[2] = p.z; nw[3] = p.w; nw[4] = q.x; nw[5] = q.y; nw[6] = q.z; nw[7] = q.w;
          }
          if (a.mod_scale) {
            const int64_t mo = (int64_t)(m < mr ? m : mr - 1) * a.ld_mod + koff[u];
            const float4 s0 = *reinterpret_cast<const float4*>(a.mod_shift + mo), s1 = *reinterpret_cast<const float4*>(a.mod_shift + mo + 4);
            const float4 c0 = *reinterpret_cast<const float4*>(a.mod_scale + mo), c1 = *reinterpret_cast<const float4*>(a.mod_scale + mo + 4);
            sh[0] = s0.x; sh[1] = s0.y; sh[2] = s0.z; sh[3] = s0.w; sh[4] = s1.x; sh[5] = s1.y; sh[6] = s1.z; sh[7] = s1.w;
            sv[0] = c0.x; sv[1] = c0.y; sv[2] = c0.z; sv[3] = c0.w; sv[4] = c1.x; sv[5] = c1.y; sv[6] = c1.z; sv[7] = c1.w;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float v = xr[m][u][j] * rstd;
            if (a.norm_w) v *= nw[j];
            if (a.mod_scale) v = v * (1.0f + sv[j]) + sh[j];
            xr[m][u][j] = v;
          }
        }
      }
    }
  }

  // ---- stream the weight rows ------------------------------------------------------------------------------------
  int parity = 0;
  while (g < n_groups) {
    const int gn = g + gstride;
    // packed fp32 FMAs (v_pk_fma_f32): the conversion delivers (k, k + 1) as a register pair, which is the FMA's operand as it stands
    vf2 pacc[RW][M], pacc2[DUAL ? RW : 1][M];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) { pacc[r][m] = vf2{0.f, 0.f}; if (DUAL) pacc2[r][m] = vf2{0.f, 0.f}; }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        vf2 w[4], w2[4];
        unpack8_mx(cur[u][r], (sc[u] >> (8 * r)) & 0xffu, w);
        if constexpr (DUAL) unpack8_mx(cur2[u][r], (sc2[u] >> (8 * r)) & 0xffu, w2);
#pragma unroll
        for (int m = 0; m < M; ++m) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const vf2 xp = {xr[m][u][2 * j], xr[m][u][2 * j + 1]};
            pacc[r][m] = __builtin_elementwise_fma(w[j], xp, pacc[r][m]);
            if constexpr (DUAL) pacc2[r][m] = __builtin_elementwise_fma(w2[j], xp, pacc2[r][m]);
          }
        }
      }
    }
    float acc[RW][M], acc2[DUAL ? RW : 1][M];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        acc[r][m] = wsum(pacc[r][m].x + pacc[r][m].y);
        if (DUAL) acc2[r][m] = wsum(pacc2[r][m].x + pacc2[r][m].y);
      }
    if (KSPLIT == 1) {
      if (lane < RW * M) {                         // every lane holds all sums: lane r * M + m keeps (r, m)
        float v = acc[0][0], v2 = DUAL ? acc2[0][0] : 0.f;
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
          for (int m = 0; m < M; ++m)
            if (lane == r * M + m) { v = acc[r][m]; if (DUAL) v2 = acc2[r][m]; }
        const int r = lane / M, m = lane - r * M;
        const int n = g * RW + r;
        if (n < N && m < mr) epi_pre(a, m, n, v, v2, eo_cur);
      }
    } else {
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < RW; ++r)
#pragma unroll
          for (int m = 0; m < M; ++m) {
            part[parity][wave][(r * M + m) * 2] = acc[r][m];
            part[parity][wave][(r * M + m) * 2 + 1] = DUAL ? acc2[r][m] : 0.f;
          }
      }
      __syncthreads();                             // g is block-uniform when KSPLIT != 1
      if (tid < RW * M) {
        const int r = tid / M, m = tid - r * M;
        const int n = g * RW + r;
        if (n < N && m < mr) {
          float s = 0.f, s2 = 0.f;
#pragma unroll
          for (int w4 = 0; w4 < NW; ++w4) { s += part[parity][w4][tid * 2]; s2 += part[parity][w4][tid * 2 + 1]; }
          epi_pre(a, m, n, s, s2, eo_cur);
        }
      }
      parity ^= 1;                                 // ping-pong: one barrier per group is enough
    }
    eo_cur = eo_nxt;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      cur[u] = nxt[u]; sc[u] = nsc[u];
      if constexpr (DUAL) { cur2[u] = nxt2[u]; sc2[u] = nsc2[u]; }
    }
    g = gn;
    if (g + gstride < n_groups) { load_eo(eo_nxt, g + gstride); issue(nxt, nxt2, nsc, nsc2, g + gstride); }   // keep two groups in flight
  }
}

// Every kernel of this file that exists, as (m, dual, ksplit, ku) - exactly what vv_gemv_mx_decide can choose: the launch ladder instantiates
// under this predicate and nothing else, and the decision checks its finished route against it.
//   whole rows (ksplit 1) at 1..5 units, the SwiGLU kernel (two code streams) at 1..4
//   4 waves splitting K at 2..5 units per wave, 8 waves at 3..5 (2 units x 8 waves is already served by 4 waves x 4 units)
//   SwiGLU with K split: 2..3 units per wave on 4 or 8 waves
constexpr bool mx_exists(int m, bool dual, int ksplit, int ku) {
  if (m != 1 && m != 2) return false;
  if (ksplit == 1) return ku >= 1 && ku <= (dual ? 4 : 5);
  if (ksplit != 4 && ksplit != 8) return false;
  if (dual) return ku == 2 || ku == 3;
  return ku >= (ksplit == 4 ? 2 : 3) && ku <= 5;
}

// persistent grid, the streaming kernel's rule: ~2 blocks per CU for the wave-per-group layout, one block per row group when the block's
// waves split K, fewer persistent blocks for long rows (every block reads all of x)
void mx_grid(const vv_lin_args& a, vv_mx_route& r) {
  const int n_groups = (a.n + RW - 1) / RW;
  const int waves = 4;
  const int work = (r.ksplit == 1) ? (n_groups + waves - 1) / waves : n_groups;
  const int cap = (r.ksplit == 1) ? 512 : (a.k > 6144 ? 512 : 1024);
  r.n_groups = n_groups;
  r.blocks = work < cap ? work : cap;
  if (g_mx_blocks > 0) r.blocks = g_mx_blocks < work ? g_mx_blocks : work;
  r.threads = r.ksplit == 1 ? 64 * waves : 64 * r.ksplit;
}

template <int M, bool DUAL, int KSPLIT, int KU>
bool launch_one(const vv_lin_args& a, const vv_mx_route& r, hipStream_t s) {
  if constexpr (mx_exists(M, DUAL, KSPLIT, KU)) {
    hipLaunchKernelGGL((gemv_mx_kernel<M, DUAL, KSPLIT, KU>), dim3(r.blocks), dim3(r.threads), 0, s, a, r.n_groups);
    return true;
  } else {
    return false;
  }
}

template <int M, bool DUAL, int KSPLIT>
bool launch_kus(const vv_lin_args& a, const vv_mx_route& r, hipStream_t s) {
  switch (r.ku) {
    case 1: return launch_one<M, DUAL, KSPLIT, 1>(a, r, s);
    case 2: return launch_one<M, DUAL, KSPLIT, 2>(a, r, s);
    case 3: return launch_one<M, DUAL, KSPLIT, 3>(a, r, s);
    case 4: return launch_one<M, DUAL, KSPLIT, 4>(a, r, s);
    case 5: return launch_one<M, DUAL, KSPLIT, 5>(a, r, s);
  }
  return false;
}

template <int M, bool DUAL>
bool launch_ks(const vv_lin_args& a, const vv_mx_route& r, hipStream_t s) {
  switch (r.ksplit) {
    case 1: return launch_kus<M, DUAL, 1>(a, r, s);
    case 4: return launch_kus<M, DUAL, 4>(a, r, s);
    case 8: return launch_kus<M, DUAL, 8>(a, r, s);
  }
  return false;
}

template <int M>
bool launch_m(const vv_lin_args& a, const vv_mx_route& r, hipStream_t s) {
  return r.dual ? launch_ks<M, true>(a, r, s) : launch_ks<M, false>(a, r, s);
}

}  // namespace

void vv_gemv_mx_set_blocks(int b) { g_mx_blocks = b; }

// The decision: which kernel of this file the call takes, and on what grid.  kind 0 = refused (vv_hip.h, VV_MXFP4: m <= 2, whole 32-blocks, a
// scale array for every matrix, 16-byte aligned codes and scales, no fragment-major flag, no bf16 hand-off) or longer than the kernels reach
// (40 units, SwiGLU 24).  Reads the arguments' values and alignments only.
vv_mx_route vv_gemv_mx_decide(const vv_lin_args& a) {
  vv_mx_route r = {};
  if (a.wdt != VV_MXFP4 || a.m < 1 || a.m > 2 || a.k % 32 || !a.wscale || (a.w2 && !a.w2scale)) return r;
  if (a.flags & (VV_LIN_W_FRAG | VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) return r;
  if ((uintptr_t)a.w % 16 || (uintptr_t)a.wscale % 16 || (a.w2 && ((uintptr_t)a.w2 % 16 || (uintptr_t)a.w2scale % 16))) return r;
  if ((uintptr_t)a.x % 16) return r;
  if (a.m > 1 && a.ldx % 4) return r;
  if (a.norm_w && (uintptr_t)a.norm_w % 16) return r;
  if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return r;
  const int units = (a.k + 511) / 512;
  const bool dual = a.w2 != nullptr;
  // smallest wave count whose per-wave slice fits the register-resident activation fragment and code streams
  int ksplit = 1, ku = units;
  if (units > (dual ? 4 : 5)) {
    const int kumax = dual ? 3 : 5;
    ksplit = 0;
    for (int w : {4, 8}) {
      if ((units + w - 1) / w <= kumax) { ksplit = w; ku = (units + w - 1) / w; break; }
    }
    if (!ksplit) return r;
  }
  r.m = a.m; r.dual = dual; r.ksplit = ksplit; r.ku = ku;
  if (!mx_exists(r.m, dual, ksplit, ku)) return r;
  mx_grid(a, r);
  r.kind = 1;
  return r;
}

int vv_launch_gemv_mx_route(const vv_lin_args& a, const vv_mx_route& r, hipStream_t s) {
  if (r.kind != 1) return 0;
  switch (r.m) {
    case 1: return launch_m<1>(a, r, s);
    case 2: return launch_m<2>(a, r, s);
  }
  return 0;
}

// the name vv_linear_route reports for this file's routes: spelled here and nowhere else
int vv_gemv_mx_route_name(const vv_mx_route& r, char* name, int cap) {
  return snprintf(name, (size_t)cap, "gemv_mx<m=%d,dual=%d,ksplit=%d,ku=%d>", r.m, r.dual, r.ksplit, r.ku);
}

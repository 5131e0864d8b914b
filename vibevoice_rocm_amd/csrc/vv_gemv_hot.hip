// vv_gemv_hot.hip — shape-specialised decode GEMVs for the six hot matrices of the 1.5B per-frame path (M = 2, bf16 weights, fp32 rows).
//
// vv_gemv_stream.hip serves every shape from one template.  The kernels here serve exactly one call site each: N, K, the row-to-wave
// assignment and the K split are compile-time constants, only the prologue and epilogue of that call site exist, and there is no row
// loop: a wave requests ALL the weight rows it owns at kernel entry (behind the activation / operand loads it needs first) and then
// consumes them in the order they were requested.
//
// The arithmetic of every output element is the generic kernel's: the same 512-element K units per lane, the same packed-FMA order
// inside a unit and over units, the same DPP reduction (vv_wave_sum), the same K-split combine order (waves 0..3), the same RMSNorm
// statistics (block-staged over 256 threads for the SwiGLU kernels, per wave for qkv) and the same fp32 epilogue expression, so the
// outputs are bit-identical to the generic path (tests/test_hip_gemv_hot.py compares with torch.equal).  What changes is only which
// wave computes which row and when its loads are issued.
//
//   kind        call site        n x k          grid x waves   rows per wave
//   hot_dual    head.gate_up     4608 x 1536    512 x 4        2 or 3  (wave w of block b: rows (512 w + b) + 2048 i: 9 rows per block)
//   hot_dual    llm.gate_up      8960 x 1536    512 x 4        4 or 5  (17 or 18 rows per block)
//   hot_down    head.down        1536 x 4608    256 x 4        6 rows per block, K split over the 4 waves (activation bytes 36.9 KB <= weight bytes 55.3 KB)
//   hot_down    llm.down         1536 x 8960    256 x 4        6 rows per block (71.7 KB <= 107.5 KB)
//   hot_rows    llm.qkv          2048 x 1536    256 x 4        2
//   hot_rows    llm.o            1536 x 1536    256 x 3        2      (the generic grid is 192 blocks: a quarter of the CUs idle)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

// ldw<NT> (vv_device.h), NT: streamed once per frame (LLM); otherwise the matrix is re-read by the next solver step (head) and stays cacheable

// one lane's 8 weights of one K unit against both activation rows: even / odd k accumulate separately (v_pk_fma_f32), j ascending
__device__ __forceinline__ void fma_unit(const u32x4 wv, const float (&x0)[8], const float (&x1)[8], vf2& p0, vf2& p1) {
  float w[8];
  unpack8(wv, w);
#pragma unroll
  for (int j = 0; j < 8; j += 2) p0 = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, vf2{x0[j], x0[j + 1]}, p0);
#pragma unroll
  for (int j = 0; j < 8; j += 2) p1 = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, vf2{x1[j], x1[j + 1]}, p1);
}

// How the arguments arrive: the leading kernel parameters are exactly what the loads in front of the first wait need, the pointers and then their
// strides as 32-bit values, at most 14 dwords.  The unit is built with kernarg preload (-mllvm -amdgpu-kernarg-preload-count=16, build.py), which has
// the command processor place those dwords in user SGPRs at wave launch: a wave's first instructions form addresses and issue global_loads instead of
// waiting for a scalar round trip to the kernarg segment.  What only the epilogue needs trails in hot_tail (a struct is passed by reference and
// never preloaded: its s_load is off the critical path).  The bodies read the arguments through hot_view under vv_lin_args' names.
struct hot_tail { float* out; int64_t ldo; int k; float eps; };
struct hot_view {     // the fields of vv_lin_args the hot bodies read, under the same names
  const float* x; int64_t ldx; const float* norm_w; float eps; const float* mod_shift; const float* mod_scale; int64_t ld_mod; const void* w; const void* w2;
  const float* bias; int k; const float* gate; int64_t gate_ld; const float* res; int64_t ldres; float* out; int64_t ldo;
};

// ---------------------------------------------------------------------------------------------------------------------------------
// SwiGLU pair (gate / up), K = 1536: RMSNorm (MOD: adaLN shift / scale on top) staged once per block over 256 threads, one weight row
// of each matrix per wave step, G = ceil(N / 2048) steps all requested at entry.
// ---------------------------------------------------------------------------------------------------------------------------------
template <int N, bool MOD, bool NT>
__global__ __launch_bounds__(256, 2) void hot_dual_kernel(const float* x, const float* norm_w, const float* mod_shift, const float* mod_scale, const void* w,
                                                          const void* w2, int ldx, int ld_mod, const hot_tail t) {
  const hot_view a{x, ldx, norm_w, t.eps, mod_shift, mod_scale, ld_mod, w, w2, nullptr, t.k, nullptr, 0, nullptr, 0, t.out, t.ldo};
  constexpr int K = 1536, KU = 3, M = 2, T = 256, NCH = 2, NCHUNKS = K / 4;
  constexpr int WAVES = 512 * 4, G = (N + WAVES - 1) / WAVES;
  constexpr bool RAGGED = (N % WAVES) != 0;      // only the last step can be past the end
  __shared__ float red[4 * M];
  __shared__ __attribute__((aligned(16))) float xs[M * KU * 512];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int gw = wave * 512 + (int)blockIdx.x;   // wave-major numbering: the rows of a ragged last step spread evenly over the blocks
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);
  const bf16_t* __restrict__ W2 = reinterpret_cast<const bf16_t*>(a.w2);

  // ---- every load the kernel makes, in the order their results are needed ----
  float4 xv[M][NCH], nv[NCH], sv[M][NCH], cv[M][NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * T;
    const int kk = ch < NCHUNKS ? ch * 4 : 0;
#pragma unroll
    for (int m = 0; m < M; ++m) xv[m][c] = *reinterpret_cast<const float4*>(a.x + (int64_t)m * a.ldx + kk);
    nv[c] = *reinterpret_cast<const float4*>(a.norm_w + kk);
    if constexpr (MOD) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const int64_t mo = (int64_t)m * a.ld_mod + kk;
        sv[m][c] = *reinterpret_cast<const float4*>(a.mod_shift + mo);
        cv[m][c] = *reinterpret_cast<const float4*>(a.mod_scale + mo);
      }
    }
  }
  u32x4 wq[G][KU], wq2[G][KU];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int n = gw + i * WAVES;
    const bool live = !RAGGED || i < G - 1 || n < N;
    // a step past the end degenerates to one 16-byte line per instruction (every lane reads element 0): no branch among the loads
    const int off = live ? n * K + lane * 8 : 0;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      wq[i][u] = ldw<NT>(W + off + (live ? u * 512 : 0));
      wq2[i][u] = ldw<NT>(W2 + off + (live ? u * 512 : 0));
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // what the prologue computes with is made opaque here, behind the weight loads (the compiler otherwise hoists arithmetic and its waits)
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
#pragma unroll
    for (int m = 0; m < M; ++m) VV_FENCE4(xv[m][c]);
    VV_FENCE4(nv[c]);
    if constexpr (MOD) {
#pragma unroll
      for (int m = 0; m < M; ++m) { VV_FENCE4(sv[m][c]); VV_FENCE4(cv[m][c]); }
    }
  }

  // ---- RMSNorm (+ modulate) once per block: thread t owns the 4-element chunks t and t + 256 of both rows ----
  float ss[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 v = xv[m][c];
      s1 += (tid + c * T < NCHUNKS) ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
    }
    ss[m] = vv_wave_sum(s1);
  }
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < M; ++m) red[wave * M + m] = ss[m];
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < M; ++m) {
    float tot = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) tot += red[w4 * M + m];
    const float rstd = rsqrtf(tot / (float)a.k + a.eps);    // a.k, not the constant: the same division as the generic kernel's
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ch = tid + c * T;
      float4 v = xv[m][c];
      v.x *= rstd; v.y *= rstd; v.z *= rstd; v.w *= rstd;
      v.x *= nv[c].x; v.y *= nv[c].y; v.z *= nv[c].z; v.w *= nv[c].w;
      if constexpr (MOD) {
        v.x = v.x * (1.0f + cv[m][c].x) + sv[m][c].x; v.y = v.y * (1.0f + cv[m][c].y) + sv[m][c].y;
        v.z = v.z * (1.0f + cv[m][c].z) + sv[m][c].z; v.w = v.w * (1.0f + cv[m][c].w) + sv[m][c].w;
      }
      if (ch < NCHUNKS) *reinterpret_cast<float4*>(&xs[(m * KU * 128 + ch) * 4]) = v;
    }
  }
  __syncthreads();
  float xr[M][KU][8];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const float4 p = *reinterpret_cast<const float4*>(&xs[m * KU * 512 + u * 512 + lane * 8]);
      const float4 q = *reinterpret_cast<const float4*>(&xs[m * KU * 512 + u * 512 + lane * 8 + 4]);
      xr[m][u][0] = p.x; xr[m][u][1] = p.y; xr[m][u][2] = p.z; xr[m][u][3] = p.w;
      xr[m][u][4] = q.x; xr[m][u][5] = q.y; xr[m][u][6] = q.z; xr[m][u][7] = q.w;
    }

  // ---- the rows, in request order ----
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int n = gw + i * WAVES;
    if (RAGGED && i == G - 1 && n >= N) break;     // wave-uniform
    vf2 p[M] = {vf2{0.f, 0.f}, vf2{0.f, 0.f}}, p2[M] = {vf2{0.f, 0.f}, vf2{0.f, 0.f}};
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      fma_unit(wq[i][u], xr[0][u], xr[1][u], p[0], p[1]);
      fma_unit(wq2[i][u], xr[0][u], xr[1][u], p2[0], p2[1]);
    }
    float acc[M], acc2[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      acc[m] = vv_wave_sum(p[m].x + p[m].y);
      acc2[m] = vv_wave_sum(p2[m].x + p2[m].y);
    }
    if (lane < M) {                                // lane m keeps (row n, m)
      const float v = lane == 0 ? acc[0] : acc[1], v2 = lane == 0 ? acc2[0] : acc2[1];
      a.out[(int64_t)lane * a.ldo + n] = vv_silu(v) * v2;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Whole-row kernel, K = 1536, two weight rows per wave, one step: llm.qkv (RMSNorm per wave, + bias) and llm.o (no prologue, + residual).
// ---------------------------------------------------------------------------------------------------------------------------------
template <int N, int WPB, bool RMS, bool NT>      // RMS: RMSNorm prologue and bias epilogue (eop = bias); else plain rows and residual epilogue (eop = res)
__global__ __launch_bounds__(64 * WPB) void hot_rows_kernel(const float* x, const float* norm_w, const float* eop, const void* w, int ldx, int ldres,
                                                            const hot_tail t) {
  const hot_view a{x, ldx, norm_w, t.eps, nullptr, nullptr, 0, w, nullptr, eop, t.k, nullptr, 0, eop, ldres, t.out, t.ldo};
  constexpr int K = 1536, KU = 3, M = 2, RW = 2;
  static_assert(N % (RW * WPB) == 0, "every wave of the grid owns one whole row pair");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = (int)blockIdx.x * WPB + wave;      // row pair
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);

  float4 xa[M][KU], xb[M][KU], na[KU], nb[KU];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float* xrow = a.x + (int64_t)m * a.ldx + lane * 8;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      xa[m][u] = *reinterpret_cast<const float4*>(xrow + u * 512);
      xb[m][u] = *reinterpret_cast<const float4*>(xrow + u * 512 + 4);
    }
  }
  if constexpr (RMS) {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      na[u] = *reinterpret_cast<const float4*>(a.norm_w + u * 512 + lane * 8);
      nb[u] = *reinterpret_cast<const float4*>(a.norm_w + u * 512 + lane * 8 + 4);
    }
  }
  // epilogue operand of output (r, m) in lane r * M + m; the other lanes fetch output 0's: no divergent branch around the load
  const int eo_id = lane < RW * M ? lane : 0;
  const int eo_r = eo_id >> 1, eo_m = eo_id & 1;
  const int eo_n = g * RW + eo_r;
  float eo;
  if constexpr (RMS) eo = a.bias[eo_n];
  else eo = a.res[(int64_t)eo_m * a.ldres + eo_n];
  u32x4 wq[RW][KU];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int u = 0; u < KU; ++u) wq[r][u] = ldw<NT>(W + (g * RW + r) * K + u * 512 + lane * 8);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < KU; ++u) {
#pragma unroll
    for (int m = 0; m < M; ++m) { VV_FENCE4(xa[m][u]); VV_FENCE4(xb[m][u]); }
    if constexpr (RMS) { VV_FENCE4(na[u]); VV_FENCE4(nb[u]); }
  }

  float xr[M][KU][8];
  float ss[M];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    ss[m] = 0.f;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      xr[m][u][0] = xa[m][u].x; xr[m][u][1] = xa[m][u].y; xr[m][u][2] = xa[m][u].z; xr[m][u][3] = xa[m][u].w;
      xr[m][u][4] = xb[m][u].x; xr[m][u][5] = xb[m][u].y; xr[m][u][6] = xb[m][u].z; xr[m][u][7] = xb[m][u].w;
      if constexpr (RMS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ss[m] = fmaf(xr[m][u][j], xr[m][u][j], ss[m]);
      }
    }
  }
  if constexpr (RMS) {
#pragma unroll
    for (int m = 0; m < M; ++m) ss[m] = vv_wave_sum(ss[m]);   // every wave holds the whole row
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float rstd = rsqrtf(ss[m] / (float)a.k + a.eps);
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const float nw[8] = {na[u].x, na[u].y, na[u].z, na[u].w, nb[u].x, nb[u].y, nb[u].z, nb[u].w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = xr[m][u][j] * rstd;
          v *= nw[j];
          xr[m][u][j] = v;
        }
      }
    }
  }

  vf2 p[RW][M];
#pragma unroll
  for (int r = 0; r < RW; ++r) {
    p[r][0] = vf2{0.f, 0.f}; p[r][1] = vf2{0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KU; ++u) fma_unit(wq[r][u], xr[0][u], xr[1][u], p[r][0], p[r][1]);
  }
  float acc[RW][M];
#pragma unroll
  for (int r = 0; r < RW; ++r)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[r][m] = vv_wave_sum(p[r][m].x + p[r][m].y);
  if (lane < RW * M) {
    const float v0 = (lane & 1) ? acc[0][1] : acc[0][0], v1 = (lane & 1) ? acc[1][1] : acc[1][0];   // lane r * M + m keeps (r, m)
    float v = (lane & 2) ? v1 : v0;
    v += eo;                                       // bias (qkv) or residual (o): one add either way
    a.out[(int64_t)eo_m * a.ldo + eo_n] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Down projection (K = 4608 / 8960): the block's 4 waves split K in interleaved 512-element units (wave w: units w, w + 4, ...) and
// combine through LDS in wave order.  A block owns R consecutive output rows, so the fp32 activation rows it reads (M x K x 4 bytes,
// once per block: each wave reads only its own K quarter) weigh less than its R x K x 2 bytes of weights; one combine per block.
//   GATE: epilogue * gate[m, n] + res[m, n] (head); else + res[m, n] (LLM)
// ---------------------------------------------------------------------------------------------------------------------------------
template <int N, int K, int R, bool GATE, bool NT>
__global__ __launch_bounds__(256) void hot_down_kernel(const float* x, const float* gate, const float* res, const void* w, int ldx, int gate_ld, int ldres,
                                                       const hot_tail t) {
  const hot_view a{x, ldx, nullptr, 0.f, nullptr, nullptr, 0, w, nullptr, nullptr, K, gate, gate_ld, res, ldres, t.out, t.ldo};
  constexpr int M = 2, NW = 4, UNITS = (K + 511) / 512, KU = (UNITS + NW - 1) / NW;
  static_assert(N % R == 0 && R * M <= 64, "whole row sets; the epilogue threads are the first R * M of the block");
  __shared__ float part[NW][R * M];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = (int)blockIdx.x * R;
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);

  int koff[KU];
  bool kval[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    koff[u] = (wave + NW * u) * 512 + lane * 8;
    kval[u] = koff[u] < K;
    if (!kval[u]) koff[u] = 0;                    // any valid address; the activation there is forced to 0
  }
  float4 xa[M][KU], xb[M][KU];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float* xrow = a.x + (int64_t)m * a.ldx;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      xa[m][u] = *reinterpret_cast<const float4*>(xrow + koff[u]);
      xb[m][u] = *reinterpret_cast<const float4*>(xrow + koff[u] + 4);
    }
  }
  // epilogue operands of output (r, m) in thread r * M + m
  const int eo_id = tid < R * M ? tid : 0;
  const int eo_r = eo_id >> 1, eo_m = eo_id & 1;
  const int eo_n = n0 + eo_r;
  float eg = 1.f;
  if constexpr (GATE) eg = a.gate[(int64_t)eo_m * a.gate_ld + eo_n];
  const float er = a.res[(int64_t)eo_m * a.ldres + eo_n];
  u32x4 wq[R][KU];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int u = 0; u < KU; ++u) wq[r][u] = ldw<NT>(W + (n0 + r) * K + koff[u]);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int m = 0; m < M; ++m) { VV_FENCE4(xa[m][u]); VV_FENCE4(xb[m][u]); }

  float xr[M][KU][8];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const bool kv = kval[u];                     // lanes past K read a valid address and contribute zeros
      xr[m][u][0] = kv ? xa[m][u].x : 0.f; xr[m][u][1] = kv ? xa[m][u].y : 0.f; xr[m][u][2] = kv ? xa[m][u].z : 0.f; xr[m][u][3] = kv ? xa[m][u].w : 0.f;
      xr[m][u][4] = kv ? xb[m][u].x : 0.f; xr[m][u][5] = kv ? xb[m][u].y : 0.f; xr[m][u][6] = kv ? xb[m][u].z : 0.f; xr[m][u][7] = kv ? xb[m][u].w : 0.f;
    }

  float acc[R][M];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    vf2 p0 = vf2{0.f, 0.f}, p1 = vf2{0.f, 0.f};
#pragma unroll
    for (int u = 0; u < KU; ++u) fma_unit(wq[r][u], xr[0][u], xr[1][u], p0, p1);
    acc[r][0] = vv_wave_sum(p0.x + p0.y);
    acc[r][1] = vv_wave_sum(p1.x + p1.y);
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < R; ++r) { part[wave][r * M] = acc[r][0]; part[wave][r * M + 1] = acc[r][1]; }
  }
  __syncthreads();
  if (tid < R * M) {
    float s = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < NW; ++w4) s += part[w4][tid];
    float v = s;
    if constexpr (GATE) v = gate_res(v, eg, er);
    else v += er;
    a.out[(int64_t)eo_m * a.ldo + eo_n] = v;
  }
}

// table order == bit order of the "gemv_hot" tuning key
constexpr int N_HOT = 6;
const vv_gemv_hot_shape g_table[N_HOT] = {
    // name           m  n     k     dual pro              mod bias gate res act             flags
    {"head.gate_up", 2, 4608, 1536, 1, VV_PRO_RMSNORM, 1, 0, 0, 0, VV_ACT_SWIGLU, VV_LIN_W_REUSED},
    {"head.down",    2, 1536, 4608, 0, VV_PRO_NONE,    0, 0, 1, 1, VV_ACT_NONE,   VV_LIN_W_REUSED},
    {"llm.gate_up",  2, 8960, 1536, 1, VV_PRO_RMSNORM, 0, 0, 0, 0, VV_ACT_SWIGLU, 0},
    {"llm.down",     2, 1536, 8960, 0, VV_PRO_NONE,    0, 0, 0, 1, VV_ACT_NONE,   0},
    {"llm.qkv",      2, 2048, 1536, 0, VV_PRO_RMSNORM, 0, 1, 0, 0, VV_ACT_NONE,   0},
    {"llm.o",        2, 1536, 1536, 0, VV_PRO_NONE,    0, 0, 0, 1, VV_ACT_NONE,   0},
};

constexpr int HOT_DEFAULT = 0x3f;   // the adopted entries (tools/mb_hot.py)
int g_hot = HOT_DEFAULT;   // tuning hook "gemv_hot": bit i = table entry i takes its hot kernel; bit 8 = the down kernels own 3 rows per block (512 blocks)

bool fits31(int64_t v) { return v >= 0 && v <= INT32_MAX; }

bool matches(const vv_gemv_hot_shape& e, const vv_lin_args& a) {
  return a.m == e.m && a.n == e.n && a.k == e.k && a.wdt == VV_BF16 && (a.w2 != nullptr) == (e.dual != 0) && a.pro == e.pro &&
         (a.pro != VV_PRO_RMSNORM || a.norm_w != nullptr) && (a.mod_scale != nullptr) == (e.mod != 0) && (!e.mod || a.mod_shift != nullptr) &&
         (a.bias != nullptr) == (e.bias != 0) && (a.gate != nullptr) == (e.gate != 0) && (!e.gate || a.gate_ld != 0) &&
         (a.res != nullptr) == (e.res != 0) && a.act == e.act && a.flags == e.flags &&
         // the kernels take the strides in front of their first loads as 32-bit values: a call they do not fit goes to the template
         fits31(a.ldx) && (!e.mod || fits31(a.ld_mod)) && (!e.gate || fits31(a.gate_ld)) && (!e.res || fits31(a.ldres));
}

}  // namespace

void vv_gemv_hot_set(int mask) { g_hot = mask < 0 ? HOT_DEFAULT : mask; }   // negative: back to the adopted set

extern "C" int vv_gemv_hot_shapes(vv_gemv_hot_shape* out, int cap) {
  for (int i = 0; i < N_HOT && i < cap; ++i) out[i] = g_table[i];
  return N_HOT;
}

// The decision: index of the enabled table entry the call equals, or -1 (the caller goes on to the generic template).  No launch, no pointer followed.
int vv_gemv_hot_covers(const vv_lin_args& a) {
  if (!(g_hot & ((1 << N_HOT) - 1)) || a.m != 2 || a.wdt != VV_BF16) return -1;
  for (int i = 0; i < N_HOT; ++i)
    if ((g_hot >> i & 1) && matches(g_table[i], a)) return i;
  return -1;
}

// The launch of table entry id (from vv_gemv_hot_covers): 1 = launched.  The caller has checked the 16-byte alignment of x, w, w2, norm_w, the
// modulation rows and ldx % 4 == 0.
int vv_launch_gemv_hot(const vv_lin_args& a, int id, hipStream_t s) {
  const bool r3 = (g_hot & 256) != 0;
  const hot_tail t{a.out, a.ldo, a.k, a.eps};
  const int ldx = (int)a.ldx, ld_mod = (int)a.ld_mod, gate_ld = (int)a.gate_ld, ldres = (int)a.ldres;   // vv_gemv_hot_covers has checked the ones the entry reads
  switch (id) {
    case 0: hipLaunchKernelGGL((hot_dual_kernel<4608, true, false>), dim3(512), dim3(256), 0, s, a.x, a.norm_w, a.mod_shift, a.mod_scale, a.w, a.w2, ldx, ld_mod, t); return 1;
    case 1:
      if (r3) hipLaunchKernelGGL((hot_down_kernel<1536, 4608, 3, true, false>), dim3(512), dim3(256), 0, s, a.x, a.gate, a.res, a.w, ldx, gate_ld, ldres, t);
      else hipLaunchKernelGGL((hot_down_kernel<1536, 4608, 6, true, false>), dim3(256), dim3(256), 0, s, a.x, a.gate, a.res, a.w, ldx, gate_ld, ldres, t);
      return 1;
    case 2: hipLaunchKernelGGL((hot_dual_kernel<8960, false, true>), dim3(512), dim3(256), 0, s, a.x, a.norm_w, a.mod_shift, a.mod_scale, a.w, a.w2, ldx, ld_mod, t); return 1;
    case 3:
      if (r3) hipLaunchKernelGGL((hot_down_kernel<1536, 8960, 3, false, true>), dim3(512), dim3(256), 0, s, a.x, a.gate, a.res, a.w, ldx, gate_ld, ldres, t);
      else hipLaunchKernelGGL((hot_down_kernel<1536, 8960, 6, false, true>), dim3(256), dim3(256), 0, s, a.x, a.gate, a.res, a.w, ldx, gate_ld, ldres, t);
      return 1;
    case 4: hipLaunchKernelGGL((hot_rows_kernel<2048, 4, true, true>), dim3(256), dim3(256), 0, s, a.x, a.norm_w, a.bias, a.w, ldx, ldres, t); return 1;
    case 5: hipLaunchKernelGGL((hot_rows_kernel<1536, 3, false, true>), dim3(256), dim3(192), 0, s, a.x, a.norm_w, a.res, a.w, ldx, ldres, t); return 1;
  }
  return 0;
}

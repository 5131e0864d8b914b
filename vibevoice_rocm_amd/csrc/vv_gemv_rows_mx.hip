// vv_gemv_rows_mx.hip — the 3 .. 8-row matrix-core GEMV (vv_gemv_rows.hip) on weight-only OCP MXFP4 weights in fragment-major order
// (VV_MXFP4_FRAG, include/vv_hip.h): the row-batched decode step and the serving sessions of a weight_quant="mxfp4" model.
//
// Roofline: HBM.  The design is gemv_rows_kernel's, restated here on its own so that not one instruction of that unit changes: a workgroup
// (g, s) = 16 weight rows x K slice s, activations fetched once per block as fp32 (requested ahead of the weights), RMSNorm statistics, norm
// weight and adaLN shift / scale, hi / lo bf16 split into LDS in fragment order, every wave's A fragments in registers, 16-byte weight loads
// straight to registers (non-temporal unless VV_LIN_W_REUSED), v_mfma_f32_16x16x32_bf16, persistent walk over row groups for the SwiGLU
// shapes with the next group's loads in flight, K slices met through write-through partial tiles and a ticket (no fence, no wait: a block
// never waits for another) or - in place, linear epilogue - through fp32 atomics, the same epilogue.
//
//   weights     codes [N / 16][K / 128][64 lanes][16 B]: dword h of lane 16 c + n of 128-wide step J of row group g holds
//               W[16 g + n][128 J + 32 h + 8 c + i] in nibble i (bits 4 i .. 4 i + 3) - the B fragment of 32-wide k step 4 J + h in the lane
//               assignment of the bf16 fragment-major layout, so one 1 KB wave load carries FOUR MFMA steps.
//   scales      bytes [N / 16][K / 128][16 rows][4 B]: byte h of the dword at ((g * K/128 + J) * 16 + n) * 4 is the E8M0 byte of block 4 J + h of
//               row 16 g + n.  An MX block (32 consecutive k of a row) is exactly one MFMA k step: one scale per B fragment, one 4-byte load
//               per lane per weight load, no table, no LDS on the decode path.
//   decode      per dword h: s = 2^(e_h - 127) built as __uint_as_float(e_h << 23); four v_cvt_scalef32_pk_bf16_fp4 (byte select 0 .. 3) give
//               the bf16x8 B fragment; value(code) * s is exact in bf16, so the products and their summation order are those of the bf16 kernel
//               on the effective matrix wherever both cut K alike.
//   KS          128-wide weight loads per wave: 4 KS A fragments (16 KS VGPRs) against 4 KS VGPRs of codes - a 4-bit weight needs four times
//               the activation registers and LDS per weight byte the bf16 form needs, which is what bounds KS (<= 4) and the K slice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned bf_bits(float f) {     // round to nearest even (finite activations)
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ float silu1(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float gelu1(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

struct RowsMxAux {
  int atomic;        // ksplit > 1, linear epilogue, res == out: every K slice adds gate * (partial [+ bias]) to out with fp32 atomics (vv_gemv_rows.hip)
  float* part;       // [n_groups][ksplit][PST] partial tiles (ksplit > 1)
  int* tickets;      // [n_groups], zero on entry, left zero
  int ksplit, spw;   // K slices per row group; 128-wide weight loads per wave
  int n_groups;
};

constexpr int MAXSPLIT = 16;

struct EpiOps { float b, g, r; };

// 8 e2m1 codes (one dword of a lane's load) under scale byte e -> the bf16 B fragment of one 32-wide k step
__device__ __forceinline__ bf16x8 mx_frag(unsigned codes, unsigned e) {
  const float s = __uint_as_float(e << 23);
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}

// KS: 128-wide weight loads per wave (KA = 4 KS activation fragments)
template <bool DUAL, int NW, int KS, bool PERS>
__global__ __launch_bounds__(NW * 64) void gemv_rows_mx_kernel(const vv_lin_args a, const RowsMxAux x) {
  constexpr int T = NW * 64;
  constexpr int KA = 4 * KS;                        // 32-wide A fragments per wave
  constexpr int NCH = (KA + 7) / 8;                 // 4-column chunks per thread per activation row
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int PST = 128 * NM + 8;                 // floats per partial tile: [NM][8][16] sums + 8 partial sums of squares
  constexpr bool MOD_OK = NCH == 1;                 // adaLN shift / scale rows: only the instantiations whose slice is one chunk per thread (registers)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* xa = reinterpret_cast<u32x4*>(smem);       // [NW][KA][64] A fragments (16 B per lane)
  __shared__ float red[PERS ? 2 : 1][NW][NM][256];  // per wave: the 16 x 16 accumulator tile(s); ping-pong when the block walks row groups
  __shared__ float ssr[NW][8];
  __shared__ float s_tot[8];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, c = lane >> 4;
  const int ks = blockIdx.y;
  const int K = a.k, N = a.n, mr = a.m;
  const int spw = x.spw, ksplit = x.ksplit, n_groups = x.n_groups;
  const int spa = 4 * spw;                          // 32-wide k steps per wave
  const int wsteps_total = K >> 7;                  // K % 128 == 0
  const int step0 = ks * NW * spa;                  // first 32-wide k step of this block
  const int k0 = step0 << 5;
  const bool rms = a.pro == VV_PRO_RMSNORM;
  const bool has_nw = rms && a.norm_w != nullptr, has_mod = MOD_OK && a.mod_scale != nullptr;
  const bool reused = (a.flags & VV_LIN_W_REUSED) != 0;

  // ---- requests, oldest first: activations, norm weight, modulation, epilogue operands, then the weights ----------------------------------
  float4 xv[8][NCH], nv[NCH], sv[8][MOD_OK ? NCH : 1], cv[8][MOD_OK ? NCH : 1];
  bool cval[NCH];
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    const int q = tid + cc * T;
    cval[cc] = q < NW * spa * 8 && (k0 + 4 * q) < K;
    const int kk = cval[cc] ? k0 + 4 * q : 4 * (tid & 7);
#pragma unroll
    for (int m = 0; m < 8; ++m) xv[m][cc] = *reinterpret_cast<const float4*>(a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx + kk);
    if (has_nw) nv[cc] = *reinterpret_cast<const float4*>(a.norm_w + kk);
    if constexpr (MOD_OK) {
      if (has_mod) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          const int64_t mo = (int64_t)(m < mr ? m : mr - 1) * a.ld_mod + kk;
          sv[m][cc] = *reinterpret_cast<const float4*>(a.mod_shift + mo);
          cv[m][cc] = *reinterpret_cast<const float4*>(a.mod_scale + mo);
        }
      }
    }
  }
  // epilogue operands of output (em, en) of a row group = thread tid < 128; absent operands read x[0] (a valid address), ignored at use
  const int em = (tid >> 4) & 7, en = tid & 15;
  const int emr = em < mr ? em : mr - 1;
  auto load_eo = [&](int grp) {
    EpiOps e;
    const int egn = min(grp, n_groups - 1) * 16 + en;               // N % 16 == 0: in bounds
    const float* pb = a.bias ? a.bias + egn : a.x;
    const float* pg = a.gate ? a.gate + (a.gate_ld ? (int64_t)emr * a.gate_ld + egn : (int64_t)egn) : a.x;
    const float* pr = a.res ? a.res + (int64_t)emr * a.ldres + egn : a.x;
    e.b = *pb; e.g = *pg; e.r = *pr;
    return e;
  };
  const int sbw = ks * NW * spw + wave * spw;       // this wave's first 128-wide weight load
  const unsigned char* __restrict__ W = reinterpret_cast<const unsigned char*>(a.w);
  const unsigned char* __restrict__ W2 = reinterpret_cast<const unsigned char*>(a.w2);
  const unsigned char* __restrict__ S = reinterpret_cast<const unsigned char*>(a.wscale);
  const unsigned char* __restrict__ S2 = reinterpret_cast<const unsigned char*>(a.w2scale);
  // a load that is not live (past the row's end, past the last row group, j >= spw) reads the first load of the matrix: a valid address
  auto issue = [&](u32x4 (&w)[KS], unsigned (&e)[KS], u32x4 (&w2)[DUAL ? KS : 1], unsigned (&e2)[DUAL ? KS : 1], int grp) {
    const bool glive = grp < n_groups;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const bool live = glive && j < spw && sbw + j < wsteps_total;
      const int64_t ld = live ? (int64_t)grp * wsteps_total + (sbw + j) : 0;
      const u32x4* p1 = reinterpret_cast<const u32x4*>(W + (ld * 64 + lane) * 16);
      const unsigned* q1 = reinterpret_cast<const unsigned*>(S + (ld * 16 + n) * 4);
      const u32x4* p2 = reinterpret_cast<const u32x4*>(W2 + (ld * 64 + lane) * 16);
      const unsigned* q2 = reinterpret_cast<const unsigned*>(S2 + (ld * 16 + n) * 4);
      if (reused) {
        w[j] = *p1; e[j] = *q1;
        if (DUAL) { w2[j] = *p2; e2[j] = *q2; }
      } else {
        w[j] = __builtin_nontemporal_load(p1); e[j] = __builtin_nontemporal_load(q1);
        if (DUAL) { w2[j] = __builtin_nontemporal_load(p2); e2[j] = __builtin_nontemporal_load(q2); }
      }
    }
  };
  const int gstride = gridDim.x;
  int g = blockIdx.x;
  u32x4 wc[KS], wc2[DUAL ? KS : 1];
  unsigned ec[KS], ec2[DUAL ? KS : 1];
  u32x4 wn[PERS ? KS : 1], wn2[(PERS && DUAL) ? KS : 1];
  unsigned en_[PERS ? KS : 1], en2[(PERS && DUAL) ? KS : 1];
  EpiOps eo = load_eo(g), eo_n = eo;
  issue(wc, ec, wc2, ec2, g);
  if constexpr (PERS) {
    eo_n = load_eo(g + gstride);
    issue(wn, en_, wn2, en2, g + gstride);
  }
  __builtin_amdgcn_sched_barrier(0);
#define VV_FENCE4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
#pragma unroll
    for (int m = 0; m < 8; ++m) VV_FENCE4(xv[m][cc]);
    if (has_nw) VV_FENCE4(nv[cc]);
    if constexpr (MOD_OK) {
      if (has_mod) {
#pragma unroll
        for (int m = 0; m < 8; ++m) { VV_FENCE4(sv[m][cc]); VV_FENCE4(cv[m][cc]); }
      }
    }
  }
#undef VV_FENCE4

  // ---- activation prologue -------------------------------------------------------------------------------------------------------------
  float rstd[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) rstd[m] = 1.0f;
  if (rms) {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      float s1 = 0.f;
#pragma unroll
      for (int cc = 0; cc < NCH; ++cc) {
        const float4 v = xv[m][cc];
        s1 += cval[cc] ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
      }
      s1 = vv_wave_sum(s1);
      if (lane == 0) ssr[wave][m] = s1;
    }
    __syncthreads();
    if (tid < 8) {
      float tot = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < NW; ++w4) tot += ssr[w4][tid];          // fixed order: deterministic
      s_tot[tid] = tot;
    }
    __syncthreads();
    if (ksplit == 1) {
#pragma unroll
      for (int m = 0; m < 8; ++m) rstd[m] = rsqrtf(s_tot[m] / (float)K + a.eps);
    }
  }
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    const int q = tid + cc * T;
    if (q >= NW * KA * 8) continue;
    const int js = q >> 3, wv = js / spa, j = js - wv * spa;        // block-relative k step -> (wave, step of the wave)
    if (wv >= NW) continue;
    const int cq = (q & 7) >> 1, half = q & 1;
    unsigned char* base = smem + ((size_t)((wv * KA + j) * 64 + cq * 16) * 16 + half * 8);
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      float4 v = xv[m][cc];
      if (rms) {
        const float r = rstd[m];
        v.x *= r; v.y *= r; v.z *= r; v.w *= r;
        if (has_nw) { v.x *= nv[cc].x; v.y *= nv[cc].y; v.z *= nv[cc].z; v.w *= nv[cc].w; }
        if constexpr (MOD_OK) {
          if (has_mod) {
            v.x = v.x * (1.0f + cv[m][cc].x) + sv[m][cc].x; v.y = v.y * (1.0f + cv[m][cc].y) + sv[m][cc].y;
            v.z = v.z * (1.0f + cv[m][cc].z) + sv[m][cc].z; v.w = v.w * (1.0f + cv[m][cc].w) + sv[m][cc].w;
          }
        }
      }
      if (!cval[cc] || m >= mr) v = make_float4(0.f, 0.f, 0.f, 0.f);
      const unsigned h0 = bf_bits(v.x), h1 = bf_bits(v.y), h2 = bf_bits(v.z), h3 = bf_bits(v.w);
      const float l0 = v.x - __uint_as_float(h0 << 16), l1 = v.y - __uint_as_float(h1 << 16);
      const float l2 = v.z - __uint_as_float(h2 << 16), l3 = v.w - __uint_as_float(h3 << 16);
      u32x2 hi, lo;
      hi.x = h0 | (h1 << 16); hi.y = h2 | (h3 << 16);
      lo.x = bf_bits(l0) | (bf_bits(l1) << 16); lo.y = bf_bits(l2) | (bf_bits(l3) << 16);
      *reinterpret_cast<u32x2*>(base + (size_t)m * 16) = hi;               // fragment row m: high parts
      *reinterpret_cast<u32x2*>(base + (size_t)(m + 8) * 16) = lo;         // fragment row m + 8: low parts
    }
  }
  __syncthreads();
  u32x4 af[KA];
#pragma unroll
  for (int j = 0; j < KA; ++j) af[j] = xa[(wave * KA + j) * 64 + lane];

  // ---- the weights meet the fragments: one row group per pass -------------------------------------------------------------------------
  int pp_ = 0;
  while (g < n_groups) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      if (j < spw && sbw + j < wsteps_total) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {      // the four 32-wide steps of the load in k order: the summation order of the bf16 kernel
          const bf16x8 b = mx_frag(wc[j][h], (ec[j] >> (8 * h)) & 0xffu);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[4 * j + h]), b, acc, 0, 0, 0);
          if (DUAL) {
            const bf16x8 b2 = mx_frag(wc2[j][h], (ec2[j] >> (8 * h)) & 0xffu);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[4 * j + h]), b2, acc2, 0, 0, 0);
          }
        }
      }
    }
    // accumulator: lane (n, c) holds fragment rows 4 c + i of weight row n
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      red[pp_][wave][0][(4 * c + i) * 16 + n] = acc[i];
      if (DUAL) red[pp_][wave][NM - 1][(4 * c + i) * 16 + n] = acc2[i];
    }
    __syncthreads();
    float s = 0.f, s2 = 0.f;
    if (tid < 128) {
#pragma unroll
      for (int w4 = 0; w4 < NW; ++w4) {
        s += red[pp_][w4][0][tid] + red[pp_][w4][0][tid + 128];               // high-part row + low-part row
        if (DUAL) s2 += red[pp_][w4][NM - 1][tid] + red[pp_][w4][NM - 1][tid + 128];
      }
    }
    float rs = 1.0f;
    if (!PERS && ksplit > 1 && x.atomic) {
      if (tid < 128) {
        const int gn = g * 16 + en;
        if (em < mr && gn < N) {
          float v = s;
          if (a.bias && ks == 0) v += eo.b;
          if (a.gate) v *= eo.g;
          atomicAdd(a.out + (int64_t)em * a.ldo + gn, v);
        }
      }
      return;
    }
    if (!PERS && ksplit > 1) {
      // partial tile out (write-through), ticket, the last block of the row group folds
      float* pp = x.part + ((int64_t)g * ksplit + ks) * PST;
      if (tid < 128) {
        __hip_atomic_store(pp + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (DUAL) __hip_atomic_store(pp + 128 + tid, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (tid < 8) __hip_atomic_store(pp + 128 * NM + tid, rms ? s_tot[tid] : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        const int tk = __hip_atomic_fetch_add(&x.tickets[g], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == ksplit - 1);
        if (s_last) __hip_atomic_store(&x.tickets[g], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
      }
      __syncthreads();
      if (!s_last) return;
      if (tid >= 128) return;
      const float* p0 = x.part + (int64_t)g * ksplit * PST;
      float pv[MAXSPLIT], pv2[DUAL ? MAXSPLIT : 1], pq[MAXSPLIT];
#pragma unroll
      for (int i = 0; i < MAXSPLIT; ++i) {                            // every partial requested before the first is used
        const int ii = i < ksplit ? i : 0;
        pv[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (DUAL) pv2[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + 128 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pq[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + 128 * NM + em, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s = 0.f; s2 = 0.f;
      float q2 = 0.f;
#pragma unroll
      for (int i = 0; i < MAXSPLIT; ++i) {
        if (i < ksplit) { s += pv[i]; if (DUAL) s2 += pv2[i]; q2 += pq[i]; }
      }
      if (rms) rs = rsqrtf(q2 / (float)K + a.eps);
    }
    if (tid < 128) {
      const int gn = g * 16 + en;
      if (em < mr && gn < N) {
        float v = s * rs, v2 = s2 * rs;
        if (a.bias) v += eo.b;
        if (a.act == VV_ACT_GELU) v = gelu1(v);
        else if (a.act == VV_ACT_SWIGLU) v = silu1(v) * v2;
        if (a.gate) v *= eo.g;
        if (a.res) v += eo.r;
        a.out[(int64_t)em * a.ldo + gn] = v;
      }
    }
    if constexpr (!PERS) {
      break;
    } else {
      g += gstride;
      pp_ ^= 1;                                        // ping-pong: one barrier per row group is enough
      eo = eo_n;
#pragma unroll
      for (int j = 0; j < KS; ++j) { wc[j] = wn[j]; ec[j] = en_[j]; if (DUAL) { wc2[j] = wn2[j]; ec2[j] = en2[j]; } }
      if (g + gstride < n_groups) {
        eo_n = load_eo(g + gstride);
        issue(wn, en_, wn2, en2, g + gstride);
      }
    }
  }
}

// the tune state of vv_gemv_rows.hip, mirrored: vv_tune sets both units together
int g_mx_rows_on = 1;          // "gemv_rows"
int g_mx_rows_blocks = 448;    // "gemv_rows_blocks": row groups x K slices aimed for before the K split stops growing
int g_mx_rows_pers = 192;      // "gemv_rows_pers": persistent blocks of the whole-row SwiGLU kernels
int g_mx_rows_atomic = 1;      // "gemv_rows_atomic": 0 = always fold K slices through the ticket (deterministic summation order)

template <bool DUAL, int NW, int KS, bool PERS>
int launch_cfg(const vv_lin_args& a, const RowsMxAux& x, int gx, hipStream_t s) {
  const size_t lds = (size_t)NW * 4 * KS * 64 * 16;   // the LDS limit of every instantiation is raised in vv_gemv_rows_mx_init (not capturable)
  hipLaunchKernelGGL((gemv_rows_mx_kernel<DUAL, NW, KS, PERS>), dim3(gx, x.ksplit), dim3(NW * 64), lds, s, a, x);
  return 1;
}

// the decision's template choice: gemv_rows_mx_kernel<dual, nw, ks, pers> and its grid
void rows_cfg(vv_rows_route& r, int dual, int nw, int ks, int pers) {
  r.dual = dual; r.nw = nw; r.ks = ks; r.pers = pers; r.f8 = 0;
  r.gx = r.n_groups;
  if (pers && r.gx > g_mx_rows_pers) {                  // the same number of row groups for every block
    const int per = (r.n_groups + g_mx_rows_pers - 1) / g_mx_rows_pers;
    r.gx = (r.n_groups + per - 1) / per;
  }
  r.kind = 1;
}

// Every kernel of this file, as (dual, nw, ks, pers) - exactly what vv_gemv_rows_mx_decide can choose
#define VV_ROWS_MX_ALL(X)                                                    \
  X(false, 8, 1, false) X(false, 8, 2, false)                                \
  X(true, 8, 1, false) X(true, 8, 2, false) X(true, 8, 1, true) X(true, 8, 2, true) \
  X(false, 4, 1, false) X(false, 4, 2, false) X(false, 4, 3, false) X(false, 4, 4, false)

}  // namespace

void vv_gemv_rows_mx_set(int on, int blocks, int pers, int atomic) {
  if (on >= 0) g_mx_rows_on = on;
  if (blocks > 0) g_mx_rows_blocks = blocks;
  if (pers > 0) g_mx_rows_pers = pers;
  if (atomic >= 0) g_mx_rows_atomic = atomic;
}

// every kernel's LDS attribute is set before any graph capture (hipFuncSetAttribute is not capturable)
int vv_gemv_rows_mx_init() {
#define VV_ROWS_MX_ATTR(D, NW, KS, P)                                                                                                   \
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemv_rows_mx_kernel<D, NW, KS, P>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                          NW * 4 * KS * 64 * 16) != hipSuccess)                                                                         \
    return vv_set_error(VV_E_HIP, "gemv_rows_mx: cannot raise the dynamic LDS limit");
  VV_ROWS_MX_ALL(VV_ROWS_MX_ATTR)
#undef VV_ROWS_MX_ATTR
  return 0;
}

// The decision (the pattern of vv_gemv_rows.hip's fp8 form, thresholds restated for 128-wide loads): which instantiation the call takes, its K
// split and grid; kind 0 = not covered.  A 128-wide load costs 4 VGPRs of codes + 1 of scale bytes per matrix and 16 of activation fragments,
// and 4 KB of LDS per wave: two loads hold the whole K <= 2048 row in 8 waves (one chunk per thread: the adaLN prologue fits), the single-matrix
// split-K form goes up to 4 loads per wave (64 fragment VGPRs, 64 KB of LDS per block).  Reads the arguments' values and alignments and the tune
// state only.
vv_rows_route vv_gemv_rows_mx_decide(const vv_lin_args& a, bool have_ws, size_t part_floats, size_t n_tickets) {
  vv_rows_route r = {};
  if (!g_mx_rows_on || a.wdt != VV_MXFP4_FRAG || !(a.flags & VV_LIN_W_FRAG) || a.m < 3 || a.m > 8 || a.n % 16 || a.n < 16 || a.k % 128 || a.k < 128) return r;
  if (a.pro == VV_PRO_SILU || (a.flags & (VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) || a.ldx == 0) return r;
  if (!a.wscale || (a.w2 && !a.w2scale)) return r;
  if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16) || (uintptr_t)a.wscale % 4 || (a.w2 && (uintptr_t)a.w2scale % 4)) return r;
  if ((uintptr_t)a.x % 16 || a.ldx % 4) return r;
  if (a.norm_w && (uintptr_t)a.norm_w % 16) return r;
  if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return r;
  const bool dual = a.w2 != nullptr;
  const int steps = a.k / 128, n_groups = a.n / 16;
  r.n_groups = n_groups; r.atomic = 0;
  if (steps <= 16) {                                  // K <= 2048: whole rows per block
    r.ksplit = 1;
    r.spw = (steps + 7) / 8;
    rows_cfg(r, dual, 8, r.spw, dual && n_groups > g_mx_rows_pers);
    return r;
  }
  if (a.mod_scale) return r;                          // the modulated prologue needs the whole row's statistic up front
  const int NW = dual ? 8 : 4, kscap = dual ? 2 : 3, ksmax = dual ? 2 : 4;
  int ksplit = 0, spw = 0;
  for (int sp = 2; sp <= MAXSPLIT && !ksplit; ++sp) {
    const int w = (steps + sp * NW - 1) / (sp * NW);
    if (w <= kscap && ((long)n_groups * sp >= g_mx_rows_blocks || w <= 1)) { ksplit = sp; spw = w; }
  }
  for (int sp = 2; sp <= MAXSPLIT && !ksplit; ++sp) {
    const int w = (steps + sp * NW - 1) / (sp * NW);
    if (w <= ksmax) { ksplit = sp; spw = w; }
  }
  if (!ksplit) return r;
  while (ksplit > 1 && (ksplit - 1) * NW * spw >= steps) --ksplit;     // drop K slices that would start past the end
  const size_t pst = dual ? 264 : 136;
  r.atomic = g_mx_rows_atomic && !dual && a.pro == VV_PRO_NONE && a.act == VV_ACT_NONE && a.res && a.res == a.out && a.ldres == a.ldo;
  if (!r.atomic && (!have_ws || (size_t)n_groups * ksplit * pst > part_floats || (size_t)n_groups > n_tickets)) return r;
  r.ksplit = ksplit; r.spw = spw;
  rows_cfg(r, dual, NW, spw, 0);
  return r;
}

// The launch of a decided route: 1 = launched, 0 = r.kind == 0 or an instantiation that is not built.  part / tickets: the split-K workspace
// the decision was told about (tickets zeroed by the caller once; every launch leaves them zero) or null.
int vv_launch_gemv_rows_mx_route(const vv_lin_args& a, const vv_rows_route& r, float* part, int* tickets, hipStream_t s) {
  if (r.kind != 1) return 0;
  RowsMxAux x;
  x.part = part; x.tickets = tickets; x.n_groups = r.n_groups; x.atomic = r.atomic; x.ksplit = r.ksplit; x.spw = r.spw;
#define VV_ROWS_MX_CASE(D, NW, KS, P) \
  if ((r.dual != 0) == D && r.nw == NW && r.ks == KS && (r.pers != 0) == P) return launch_cfg<D, NW, KS, P>(a, x, r.gx, s);
  VV_ROWS_MX_ALL(VV_ROWS_MX_CASE)
#undef VV_ROWS_MX_CASE
  return 0;
}

// the name vv_linear_route reports for this file's route: spelled here and nowhere else
int vv_gemv_rows_mx_route_name(const vv_rows_route& r, char* name, int cap) {
  return snprintf(name, (size_t)cap, "gemv_rows_mx<dual=%d,nw=%d,ks=%d,pers=%d> ksplit=%d atomic=%d", r.dual, r.nw, r.ks, r.pers, r.ksplit, r.atomic);
}

// decide + launch: 1 launched, 0 not covered (the caller falls back), < 0 error
int vv_launch_gemv_rows_mx(const vv_lin_args& a, float* part, size_t part_floats, int* tickets, size_t n_tickets, hipStream_t s) {
  return vv_launch_gemv_rows_mx_route(a, vv_gemv_rows_mx_decide(a, part && tickets, part_floats, n_tickets), part, tickets, s);
}

// vv_gemv_mx6.hip — the batch-1/2 weight-streaming GEMV on VV_MXFP6 weights (OCP MXFP6 e2m3 codes + one E8M0 scale byte per 32 k of a row).
//
// Roofline: HBM, 0.78 bytes per weight.  The structure is the streaming GEMV's (vv_gemv_stream.hip): weights go from HBM into VGPRs with
// non-temporal loads (nothing is shared between waves, no LDS round trip), a lane's activation slice lives in registers for the whole kernel
// (prologue = RMSNorm / adaLN modulate / SiLU fused), the workgroups are persistent and every wave keeps a row group's worth of loads in
// flight while it reduces the rows that have arrived (a ring of code rows, below), sums fold in a fixed order (no atomics), each output's
// epilogue runs in a lane of its own.  The one LDS round trip is the prologue's: it loads in a coalesced arrangement and transposes its result.
//
// What differs is the geometry, because the decode differs: ONE v_cvt_scalef32_pk32_f32_fp6 turns the 24 bytes of a whole 32-block of one row
// and its block scale 2^(e - 127), built as __uint_as_float(e << 23), into 32 scaled fp32 weights.  So a lane owns 32-BLOCKS, not 8-wide slices:
//   lane l of a wave owns block 64 s + l of a row for each of its KU slots s; a unit is 64 blocks = 2048 k
//   a row group is FOUR weight rows; the lane decodes its block of each of them against the same 32 x M activations it holds
//   a block's 24 bytes come as one 16-byte and one 8-byte load from two planes (layout: include/vv_hip.h), each contiguous across the wave,
//   and the four rows' scale bytes of the lane's block as one 4-byte load
// Registers set the shape: 32 x M activations per unit next to one row group's codes (4 rows x 6 dwords, two weight streams for SwiGLU) and the 32
// decoded weights of the block at hand.  The compiler's report (profiles/mxfp6_gemv.txt) admits ONE unit per wave: at two (KU = 2) the m = 2
// kernel spilled 137 VGPRs.  KU stays a template argument of the kernel and of the route's name; only KU = 1 is built.
//   KSPLIT == 1         K <= 2048: a wave owns whole rows (block = 4 independent waves)
//   KSPLIT == 2 .. 12   the block's waves split K: wave w owns unit w, and the sums combine through LDS in wave order.  Up to 8 waves a
//                       block's lanes may hold 256 VGPRs, which the SwiGLU kernel (two code streams) needs: K <= 16384; one weight stream fits
//                       the 168 of a 10- or 12-wave block: K <= 24576 (the 7B down-projection, K = 18944: 10 waves)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

typedef unsigned int u32x6 __attribute__((ext_vector_type(6)));
typedef float f32x32 __attribute__((ext_vector_type(32)));

// the epilogue operands (bias / gate / residual) of one output are fetched a row group ahead: EpiOp<false>, epi_load (vv_device.h)
__device__ __forceinline__ void epi_store(const vv_lin_args& a, int m, int n, float v, float v2, const EpiOp<false>& e) {
  a.out[(int64_t)m * a.ldo + n] = vv_epi_value(a, v, v2, e);
}

// the 32 weights of one block: its 24 bytes (16 from plane A, 8 from plane B) under scale byte e
__device__ __forceinline__ f32x32 decode32(const u32x4 lo, const u32x2 hi, unsigned int e) {
  const u32x6 c = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y};
  return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(c, __uint_as_float(e << 23));
}

int g_blocks_override = 0;   // tuning hook "gemv_blocks" (vv_tune), shared with the streaming GEMV

constexpr int RW = 4;        // weight rows per row group (the layout's, vv_hip.h)

template <int M, bool DUAL, int KSPLIT, int KU>
__global__ __launch_bounds__(KSPLIT == 1 ? 256 : 64 * KSPLIT) void gemv_mx6_kernel(const vv_lin_args a, const int n_groups) {
  constexpr int NW = (KSPLIT == 1) ? 4 : KSPLIT;     // waves per block
  __shared__ float red[NW * M];
  __shared__ float part[2][NW][RW * M * 2];
  __shared__ __attribute__((aligned(16))) float tp[NW][64 * 20];      // per wave: the prologue's transposition slab (below)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // uniform, and known to be
  const int K = a.k, N = a.n, mr = a.m;              // mr <= M real rows
  const int nb = K >> 5;                             // 32-blocks per row
  const unsigned char* __restrict__ C1 = reinterpret_cast<const unsigned char*>(a.w);
  const unsigned char* __restrict__ C2 = reinterpret_cast<const unsigned char*>(a.w2);
  const unsigned char* __restrict__ S1 = reinterpret_cast<const unsigned char*>(a.wscale);
  const unsigned char* __restrict__ S2 = reinterpret_cast<const unsigned char*>(a.w2scale);

  // ---- this lane's blocks ------------------------------------------------------------------------------------------
  unsigned int kb[KU];
  bool kval[KU];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const int b = ((KSPLIT == 1 ? 0 : wave) * KU + u) * 64 + lane;
    kval[u] = b < nb;
    kb[u] = kval[u] ? (unsigned int)b : 0u;          // any valid block; the activations there are forced to 0
  }
  const bool reused = (a.flags & VV_LIN_W_REUSED) != 0;
  const int gstride = (KSPLIT == 1) ? gridDim.x * NW : gridDim.x;
  int g = (KSPLIT == 1) ? blockIdx.x * NW + wave : blockIdx.x;      // wave-uniform (made so above), so a group's base address is scalar
  const int64_t gbytes = (int64_t)nb * (RW * 24);    // a row group's codes: plane A [4][nb][16], then plane B [4][nb][8]
  const int64_t pb_off = (int64_t)nb * (RW * 16);

  // A ring of NBUF rows of codes (per weight stream): the moment a row's registers are decoded they are asked to receive the row NBUF
  // further on - of this group or of the wave's next one - so a wave always has NBUF rows in flight at 6 dwords each.  A whole group where
  // the registers allow; half a group in the kernels at their limit: two weight streams against two activation rows (256 VGPRs), and the 10-
  // and 12-wave blocks (168)
  constexpr int D = DUAL ? 2 : 1;
  constexpr int NBUF = ((DUAL && M == 2) || KSPLIT > 8) ? 2 : RW;
  u32x4 bufA[D][NBUF][KU];
  u32x2 bufB[D][NBUF][KU];
  unsigned int bufS[D][KU], nxtS[D][KU];
  // addresses: a scalar base per (group, row, plane) plus this lane's 32-bit byte offset (block index x 16 / 8 / 4)
  auto issue_row = [&](int grp, int r, auto nt) {      // row r of group grp into its ring slot; nt: non-temporal (streamed once) or cacheable (VV_LIN_W_REUSED)
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const unsigned char* pa = (d ? C2 : C1) + grp * gbytes + (int64_t)r * nb * 16;
      const unsigned char* pb = (d ? C2 : C1) + grp * gbytes + pb_off + (int64_t)r * nb * 8;
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const u32x4* qa = reinterpret_cast<const u32x4*>(pa + kb[u] * 16u);
        const u32x2* qb = reinterpret_cast<const u32x2*>(pb + kb[u] * 8u);
        if constexpr (decltype(nt)::value) { bufA[d][r % NBUF][u] = __builtin_nontemporal_load(qa); bufB[d][r % NBUF][u] = __builtin_nontemporal_load(qb); }
        else { bufA[d][r % NBUF][u] = *qa; bufB[d][r % NBUF][u] = *qb; }
      }
    }
  };
  auto issue_first = [&](int grp, auto nt) {
#pragma unroll
    for (int r = 0; r < NBUF; ++r) issue_row(grp, r, nt);
  };
  auto issue_scales = [&](unsigned int (&S)[D][KU], int grp) {
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int u = 0; u < KU; ++u) S[d][u] = *reinterpret_cast<const unsigned int*>((d ? S2 : S1) + (int64_t)grp * nb * 4 + kb[u] * 4u);
  };
  // epilogue: output (r, m) of a row group belongs to lane / thread r * M + m (KSPLIT == 1: lane of the wave that owns the group; K split:
  // thread of the block), which fetches the next group's operands right after its store: they arrive behind that group's codes, which the
  // wave has consumed by the time it needs them
  const bool has_eo = a.bias || a.gate || a.res;
  const int eid = (KSPLIT == 1) ? lane : tid;
  const int eo_id = eid < RW * M ? eid : 0;          // lanes that own no output fetch output 0's operands: no divergent branch around the loads
  const int eo_r = eo_id / M, eo_m = (eo_id - eo_r * M) < mr ? (eo_id - eo_r * M) : mr - 1;
  EpiOp<false> eo_cur = {{0.f, 1.f, 0.f}};
  auto load_eo = [&](EpiOp<false>& e, int grp) {
    if (has_eo) e = epi_load<false>(a, eo_m, min(grp * RW + eo_r, N - 1));
  };

  // ---- activations: this lane's 32 k of every unit, after the prologue, as the packed FMA's operand pairs ---------------------------
  // The prologue runs in a COALESCED arrangement - lane l holds the 4-float chunks c = 64 j + l (j = 0..7) of the wave's unit, so every load of
  // x, the norm weight and the adaLN rows is 1 KB contiguous per wave - and only its result is transposed, through a per-wave LDS slab, into
  // the arrangement the decode needs (lane l: chunks 8 l .. 8 l + 7, its block).  Loading straight into that arrangement made every float4
  // load touch 64 cache lines, 56 such loads per wave in the adaLN-modulated SwiGLU kernel: 15.1 us on the 1.5B head's gate / up pair against
  // 10.6 us this way (profiles/mxfp6_gemv.txt).  Everything the prologue does but the row statistics is elementwise, so the arrangement does
  // not matter to it.
  // Every load it can issue up front - the x rows, the norm weight - goes out in ONE batch AHEAD of the first row group's codes: loads return
  // in order, these are L2 hits and come back first, so the statistics and the normalisation run while the codes are in flight.
  const bool rms = a.pro == VV_PRO_RMSNORM, has_nw = rms && a.norm_w, has_mod = rms && a.mod_scale;
  unsigned int co[KU][8];                            // float offset of chunk j of unit u, 0 (a valid address) past K
  bool cval[KU][8];
#pragma unroll
  for (int u = 0; u < KU; ++u)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k0 = ((KSPLIT == 1 ? 0 : wave) * KU + u) * 2048 + (j * 64 + lane) * 4;
      cval[u][j] = k0 < K;
      co[u][j] = cval[u][j] ? (unsigned int)k0 : 0u;
    }
  float4 xv[M][KU][8], nw[KU][8];
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const float* xrow = a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx;
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) xv[m][u][j] = *reinterpret_cast<const float4*>(xrow + co[u][j]);
  }
  if (has_nw) {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) nw[u][j] = *reinterpret_cast<const float4*>(a.norm_w + co[u][j]);
  } else {
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) nw[u][j] = make_float4(1.f, 1.f, 1.f, 1.f);
  }
  // the first rows of the first group (a wave without a group reads group 0: always inside the matrix)
  {
    const int g0 = g < n_groups ? g : 0;
    load_eo(eo_cur, g0);
    issue_scales(bufS, g0);
    if (reused) issue_first(g0, std::false_type{});
    else issue_first(g0, std::true_type{});
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        VV_FENCE4(xv[m][u][j]);                      // nothing of the arithmetic below moves in front of the code requests
        if (!cval[u][j]) xv[m][u][j] = make_float4(0.f, 0.f, 0.f, 0.f);      // a chunk past K read chunk 0: it contributes zeros
      }
  if (a.pro == VV_PRO_SILU) {
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float4& p = xv[m][u][j];
          p.x = vv_silu(p.x); p.y = vv_silu(p.y); p.z = vv_silu(p.z); p.w = vv_silu(p.w);
        }
  }
  if (rms) {
    float ss[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float t = 0.f;
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float4 p = xv[m][u][j];
          t = fmaf(p.x, p.x, t); t = fmaf(p.y, p.y, t); t = fmaf(p.z, p.z, t); t = fmaf(p.w, p.w, t);
        }
      ss[m] = vv_wave_sum(t);                               // KSPLIT == 1: the wave holds the whole row
    }
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
        for (int w = 0; w < NW; ++w) ss[m] += red[w * M + m];      // wave order: deterministic
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const float rstd = rsqrtf(ss[m] / (float)K + a.eps);
#pragma unroll
      for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float4& p = xv[m][u][j];
          p.x = p.x * rstd * nw[u][j].x; p.y = p.y * rstd * nw[u][j].y; p.z = p.z * rstd * nw[u][j].z; p.w = p.w * rstd * nw[u][j].w;
        }
    }
    if (has_mod) {                                   // adaLN: a row's scale and shift of the wave's unit in one batch of loads (two in the
      constexpr int MB = KSPLIT > 8 ? 4 : 8;         // 10- and 12-wave blocks, whose lanes have 168 registers)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float* pc = a.mod_scale + (int64_t)(m < mr ? m : mr - 1) * a.ld_mod;
        const float* ps = a.mod_shift + (int64_t)(m < mr ? m : mr - 1) * a.ld_mod;
#pragma unroll
        for (int u = 0; u < KU; ++u)
#pragma unroll
          for (int j0 = 0; j0 < 8; j0 += MB) {
            float4 c[MB], s[MB];
#pragma unroll
            for (int j = 0; j < MB; ++j) {
              c[j] = *reinterpret_cast<const float4*>(pc + co[u][j0 + j]);
              s[j] = *reinterpret_cast<const float4*>(ps + co[u][j0 + j]);
            }
#pragma unroll
            for (int j = 0; j < MB; ++j) {
              float4& p = xv[m][u][j0 + j];
              p.x = p.x * (1.0f + c[j].x) + s[j].x; p.y = p.y * (1.0f + c[j].y) + s[j].y;
              p.z = p.z * (1.0f + c[j].z) + s[j].z; p.w = p.w * (1.0f + c[j].w) + s[j].w;
              if (!cval[u][j0 + j]) p = make_float4(0.f, 0.f, 0.f, 0.f);      // a chunk past K: the shift must not count
            }
            __builtin_amdgcn_sched_barrier(0);       // one batch at a time: the next one's loads would double the registers
          }
      }
    }
  }
  // the transposition, half a unit at a time: half h moves chunks 4 h .. 4 h + 3 of every lane's block.  A lane holds chunks 64 j + l, whose
  // place inside their block is l & 7, so the lanes with bit 2 of l equal to h write all eight of theirs and every lane reads four.  A block's
  // four chunks lie 80 bytes from its neighbour's (20 dwords: 16 lanes' 16-byte reads fall into 16 different bank quads).  A wave's LDS
  // operations complete in order and nothing but this wave touches its slab, so wave barriers (no instruction: they only hold the compiler's
  // order) are all it takes
  vf2 xr[M][KU][16];
  float* slab = tp[wave];
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (((lane >> 2) & 1) == h) {
#pragma unroll
          for (int j = 0; j < 8; ++j) *reinterpret_cast<float4*>(slab + (j * 8 + (lane >> 3)) * 20 + (lane & 3) * 4) = xv[m][u][j];
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 v = *reinterpret_cast<const float4*>(slab + lane * 20 + j * 4);
          xr[m][u][2 * (4 * h + j)] = vf2{v.x, v.y};
          xr[m][u][2 * (4 * h + j) + 1] = vf2{v.z, v.w};
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_sched_barrier(0);           // half by half: interleaved, the halves hold both arrangements of every row at once
      }

  // ---- stream the weight rows ------------------------------------------------------------------------------------------------------
  int parity = 0;
  while (g < n_groups) {
    const int gn = g + gstride;
    const bool more = gn < n_groups;                 // wave-uniform
    if (more) issue_scales(nxtS, gn);              // ahead of the codes they scale
    float own = 0.f, own2 = 0.f;                     // KSPLIT == 1: the sums of the output this lane owns
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      // even and odd k of a lane accumulate separately on packed FMAs (v_pk_fma_f32) and are added once per row
      vf2 pacc[M], pacc2[M];
#pragma unroll
      for (int m = 0; m < M; ++m) { pacc[m] = vf2{0.f, 0.f}; pacc2[m] = vf2{0.f, 0.f}; }
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const f32x32 w = decode32(bufA[0][r % NBUF][u], bufB[0][r % NBUF][u], (bufS[0][u] >> (8 * r)) & 0xffu);
        f32x32 w2;
        if constexpr (DUAL) w2 = decode32(bufA[D - 1][r % NBUF][u], bufB[D - 1][r % NBUF][u], (bufS[D - 1][u] >> (8 * r)) & 0xffu);
        if (u == KU - 1) {                           // the codes of row r are weights now: their registers take the row NBUF further on
          const bool here = r + NBUF < RW;           // ... of this group, or of the wave's next one if it has one
          const int grp = here ? g : gn, row = (r + NBUF) % RW;
          if (here || more) {
            if (reused) issue_row(grp, row, std::false_type{});
            else issue_row(grp, row, std::true_type{});
          }
        }
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            pacc[m] = __builtin_elementwise_fma(vf2{w[2 * j], w[2 * j + 1]}, xr[m][u][j], pacc[m]);
            if constexpr (DUAL) pacc2[m] = __builtin_elementwise_fma(vf2{w2[2 * j], w2[2 * j + 1]}, xr[m][u][j], pacc2[m]);
          }
      }
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const float s = vv_wave_sum(pacc[m].x + pacc[m].y);
        const float s2 = DUAL ? vv_wave_sum(pacc2[m].x + pacc2[m].y) : 0.f;
        if (KSPLIT == 1) {
          if (lane == r * M + m) { own = s; own2 = s2; }
        } else if (lane == 0) {
          part[parity][wave][(r * M + m) * 2] = s;
          part[parity][wave][(r * M + m) * 2 + 1] = s2;
        }
      }
    }
    if (KSPLIT == 1) {
      if (lane < RW * M) {
        const int r = lane / M, m = lane - r * M;
        const int n = g * RW + r;
        if (n < N && m < mr) epi_store(a, m, n, own, own2, eo_cur);
      }
    } else {
      __syncthreads();                               // g is block-uniform when K is split
      if (tid < RW * M) {
        const int r = tid / M, m = tid - r * M;
        const int n = g * RW + r;
        if (n < N && m < mr) {
          float s = 0.f, s2 = 0.f;
#pragma unroll
          for (int w = 0; w < NW; ++w) { s += part[parity][w][tid * 2]; s2 += part[parity][w][tid * 2 + 1]; }      // wave order: deterministic
          epi_store(a, m, n, s, s2, eo_cur);
        }
      }
      parity ^= 1;                                   // ping-pong: one barrier per group is enough
    }
    if (more) load_eo(eo_cur, gn);
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
      for (int u = 0; u < KU; ++u) bufS[d][u] = nxtS[d][u];
    g = gn;
  }
}

// Every kernel of this file, as X(M, DUAL, KSPLIT, KU): the one list the launch and the decision's check read (the kernels use static LDS only
// and need no attribute set-up).  Whole rows (KSPLIT 1) and 2..6 or 8 waves splitting K; 10 and 12 waves for one weight stream.
#define VV_MX6_SPLITS(X, M, DUAL) X(M, DUAL, 1, 1) X(M, DUAL, 2, 1) X(M, DUAL, 3, 1) X(M, DUAL, 4, 1) X(M, DUAL, 5, 1) X(M, DUAL, 6, 1) X(M, DUAL, 8, 1)
#define VV_MX6_LONG(X, M) X(M, false, 10, 1) X(M, false, 12, 1)
#define VV_MX6_KERNELS(X) \
  VV_MX6_SPLITS(X, 1, false) VV_MX6_SPLITS(X, 1, true) VV_MX6_SPLITS(X, 2, false) VV_MX6_SPLITS(X, 2, true) VV_MX6_LONG(X, 1) VV_MX6_LONG(X, 2)

constexpr bool mx6_exists(int m, bool dual, int ksplit, int ku) {
#define X(M_, D_, KS_, KU_) if (m == M_ && dual == D_ && ksplit == KS_ && ku == KU_) return true;
  VV_MX6_KERNELS(X)
#undef X
  return false;
}

}  // namespace

void vv_gemv_mx6_set_blocks(int b) { g_blocks_override = b; }

// The one copy of what a VV_MXFP6 call must be (vv_hip.h): 0 = taken, else the reason it is refused (VV_E_UNSUPPORTED).  Reads values and alignments only.
const char* vv_gemv_mx6_refusal(const vv_lin_args& a, int*) {
  if (a.flags & (VV_LIN_W_FRAG | VV_LIN_X_BF16 | VV_LIN_OUT_BF16 | VV_LIN_W_MXGEMM)) return "no VV_LIN_W_FRAG, bf16 hand-off or VV_LIN_W_MXGEMM";
  if (a.m < 1 || a.m > 2) return "m <= 2";
  if (a.k % 32) return "k % 32 == 0";
  if (!a.wscale || (a.w2 && !a.w2scale)) return "scale bytes for w (and w2)";
  if ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16)) return "16-byte aligned codes";
  if ((uintptr_t)a.wscale % 4 || (a.w2 && (uintptr_t)a.w2scale % 4)) return "4-byte aligned scale bytes";
  if ((uintptr_t)a.x % 16 || (a.m > 1 && a.ldx % 4)) return "16-byte aligned activation rows";
  if (a.norm_w && (uintptr_t)a.norm_w % 16) return "a 16-byte aligned norm weight";
  if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return "16-byte aligned modulation rows";
  if (a.k > (a.w2 ? 8 : 12) * 2048) return "k <= 24576 (SwiGLU: 16384)";
  return nullptr;
}

// The decision: kind 0 = refused (vv_gemv_mx6_refusal says why).  One wave per 2048-wide unit of the row; 7 waves run as 8, 9 as 10, 11 as 12.
vv_mx6_route vv_gemv_mx6_decide(const vv_lin_args& a) {
  vv_mx6_route r = {};
  if (vv_gemv_mx6_refusal(a, nullptr)) return r;
  const int units = (a.k + 2047) / 2048;
  r.m = a.m; r.dual = a.w2 != nullptr; r.ku = 1;
  r.ksplit = units <= 6 ? units : (units + 1) & ~1;
  if (!mx6_exists(r.m, r.dual != 0, r.ksplit, r.ku)) return r;
  // persistent grid: a CU keeps 8 waves of these kernels (12 of the 10- and 12-wave blocks') - 2048 on the chip; whole rows: blocks of 4 waves, one group per wave
  // and round; K split: one block per row group and round
  r.n_groups = (a.n + RW - 1) / RW;
  const int work = r.ksplit == 1 ? (r.n_groups + 3) / 4 : r.n_groups;
  const int cap = r.ksplit == 1 ? 512 : 2048 / r.ksplit;
  r.blocks = work < cap ? work : cap;
  if (g_blocks_override > 0) r.blocks = g_blocks_override < work ? g_blocks_override : work;
  r.threads = r.ksplit == 1 ? 256 : 64 * r.ksplit;
  r.kind = 1;
  return r;
}

int vv_launch_gemv_mx6_route(const vv_lin_args& a, const vv_mx6_route& r, hipStream_t s) {
  if (!r.kind) return 0;
#define X(M_, D_, KS_, KU_)                                                                                                             \
  if (r.m == M_ && (r.dual != 0) == D_ && r.ksplit == KS_ && r.ku == KU_) {                                                            \
    hipLaunchKernelGGL((gemv_mx6_kernel<M_, D_, KS_, KU_>), dim3(r.blocks), dim3(r.threads), 0, s, a, r.n_groups);                     \
    return 1;                                                                                                                           \
  }
  VV_MX6_KERNELS(X)
#undef X
  return 0;
}

// the names vv_linear_route reports for this file's routes: spelled here and nowhere else
int vv_gemv_mx6_route_name(const vv_mx6_route& r, char* name, int cap) {
  return snprintf(name, (size_t)cap, "gemv_mx6<m=%d,dual=%d,ksplit=%d,ku=%d>", r.m, r.dual, r.ksplit, r.ku);
}

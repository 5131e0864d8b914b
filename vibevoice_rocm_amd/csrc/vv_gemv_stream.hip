// vv_gemv_stream.hip — the batch-1/2 weight-streaming GEMV of the per-frame path (bf16 weights, M <= 4 rows).
//
// Roofline: HBM.  Every weight byte is read once per call with non-temporal 16-byte loads straight into VGPRs
// (no LDS round trip: nothing is shared between waves), the activation slice each lane needs lives in registers
// for the whole kernel (prologue = RMSNorm / adaLN modulate / SiLU fused, computed once per wave), and the
// workgroups are persistent: each wave walks its row groups with the next group's loads already in flight while
// it reduces the current one (register double buffering), so the memory pipe never drains between rows.
// Row sums use DPP row reductions (vv_wave_sum), every output's epilogue (bias / GELU / SwiGLU / gate / residual) runs in its own
// lane on operands fetched one row group ahead, M <= 2 has an fp8 (e4m3fn codes + row scale), an NF4 (4-bit codes + per-64 block
// scale, see below) and an MXFP4 (OCP e2m1 codes + one E8M0 scale byte per 32 k of a row, see below) instantiation, M = 8 covers the T = 8
// conv stage when K splits to <= 2 units per wave.
//   KSPLIT == 1        a wave owns RW whole weight rows per step (block = 4 independent waves)        K <= 2560
//   KSPLIT == 4/8/16   the block's 4/8/16 waves split K (interleaved 512-element units) and combine through LDS
//                      in a fixed order (long K: 1.5B down-projections, every 7B matrix); MXFP4: 4 / 8 waves, K <= 2560 whole (SwiGLU: 2048)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "vv_hip.h"
#include "vv_common.h"
#include "vv_device.h"

namespace {

// 8 e4m3fn weights in the low 8 bytes of the tile register (fp8 weight-only mode: 8-byte loads per lane)
__device__ __forceinline__ void unpack8_f8(const u32x4 v, float (&o)[8]) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
  o[0] = a.x; o[1] = a.y; o[2] = b.x; o[3] = b.y; o[4] = c.x; o[5] = c.y; o[6] = d.x; o[7] = d.y;
}

// epilogue operands (bias / adaLN gate / residual) of one output are loaded one row group ahead, in front of the weight loads that follow them in
// the queue: EpiOp<ROWSC>, epi_load (vv_device.h).  ROWSC: the instantiation can meet fp8 row scales at all (every format but MXFP4).  For the
// others the fp8 loads and multiplies hang on the run-time test a.wdt == VV_FP8; the MXFP4 kernels carry none of them: their EpiOp is b, g, r.
__device__ __forceinline__ EpiOp<true> epi_load_cond(const vv_lin_args& a, int m, int n) {   // one uniform branch per operand (owner lanes only)
  EpiOp<true> e;
  e.b = a.bias ? a.bias[n] : 0.f;
  e.g = a.gate ? (a.gate_ld ? a.gate[(int64_t)m * a.gate_ld + n] : a.gate[n]) : 1.f;
  e.r = a.res ? a.res[(int64_t)m * a.ldres + n] : 0.f;
  e.s = (a.wdt == VV_FP8) ? a.wscale[n] : 1.f;
  e.s2 = (a.wdt == VV_FP8 && a.w2) ? a.w2scale[n] : 1.f;
  return e;
}
template <bool ROWSC>
__device__ __forceinline__ void epi_pre(const vv_lin_args& a, int m, int n, float v, float v2, const EpiOp<ROWSC>& e) {
  if constexpr (ROWSC) {
    if (a.wdt == VV_FP8) { v *= e.s; if (a.w2) v2 *= e.s2; }      // fp8 codes carry a row scale
  }
  a.out[(int64_t)m * a.ldo + n] = vv_epi_value(a, v, v2, e);
}

// NF4 (VV_NF4, weight-only 4-bit): the instantiation streams FOUR weight rows per step so that each lane's 16-byte load carries the 32 codes
// of its own 8-wide k slice of one 512-wide unit in each of the 4 rows (codes [N/4][K/512][64 lanes][4 rows][8 nibbles], include/vv_hip.h).
// Decode: every (row, 64-block) of a unit pair gets its 16-entry table bf16(table[c] * absmax) built ONCE by one lane (lane = table index:
// 16 multiplies and 8 packed converts, which also do the bf16 rounding the definition asks for) into the wave's LDS slot; every weight is
// then one nibble extract, one ds_read_u16 and one shift into the high half of an fp32.  The scales of a unit pair are one 4-byte load per lane.
__constant__ float c_nf4_table[16] = {-1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f,
                                      -0.18477343022823334f, -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f,
                                      0.24611230194568634f, 0.33791524171829224f, 0.44070982933044434f, 0.5626170039176941f,
                                      0.7229568362236023f, 1.0f};
__device__ __forceinline__ void nf4_build_lut(float s, unsigned int* dst) {   // dst: this lane's 8 dwords (16 bf16) in the wave's LDS slot
  unsigned int e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x2 v = {c_nf4_table[2 * j] * s, c_nf4_table[2 * j + 1] * s};
    e[j] = __builtin_bit_cast(unsigned int, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32: round to nearest even
  }
  *reinterpret_cast<u32x4*>(dst) = u32x4{e[0], e[1], e[2], e[3]};
  *reinterpret_cast<u32x4*>(dst + 4) = u32x4{e[4], e[5], e[6], e[7]};
}

// MXFP4 (VV_MXFP4, weight-only OCP Microscaling FP4): the NF4 geometry - a row group is FOUR weight rows, a lane's 16-byte load carries the 32
// codes of its own 8-wide k slice of one 512-wide unit in each of the 4 rows (layout: include/vv_hip.h) - and one 4-byte load per unit carries
// the four rows' scale bytes of the lane's 32-block.  Decode is the vector ALU's own: v_cvt_scalef32_pk_f32_fp4 turns one byte (two codes) and
// the block scale 2^(e - 127), built as __uint_as_float(e << 23), into two scaled fp32 weights - four per dword of codes, no table, no LDS.

// The 8 weights of one dword of codes (nibble i = k0 + i) under scale byte e: byte b of the dword holds k0 + 2 b (low nibble) and k0 + 2 b + 1
__device__ __forceinline__ void unpack8_mx(unsigned int c, unsigned int e, vf2 (&w)[4]) {
  const float s = __uint_as_float(e << 23);
  w[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 0);
  w[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 1);
  w[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 2);
  w[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(c, s, 3);
}
// The MXFP4 kernels were written against one setting of the "gemv_opt" tune word and never read it: batched prologue for RMSNorm (bit 0) and
// for no prologue (bit 1), straight-line epilogue-operand loads (bit 2); no block-staged prologue (bit 3: their dual whole-row kernels take
// the per-wave paths, so no staging buffer sits in their LDS) and no forced cacheable loads (bit 4).  Their registers and grids were sized
// under that policy, so it is a compile-time constant for them; note that it is NOT the library default (13) the other formats run under.
constexpr int MX_OPT = 7;

int g_blocks_override = 0;   // tuning hook (vv_tune)
int g_waves_override = 0;    // tuning hook "gemv_waves": waves per block of the whole-row (KSPLIT == 1) kernels, 3 .. 8
int g_opt = 13;              // tuning hook "gemv_opt": bit 0 / 1 = batched prologue for RMSNorm / no prologue, bit 2 = straight-line epilogue-operand loads, bit 3 = block-staged RMSNorm prologue (KSPLIT == 1)
int g_long_cap = 512;        // persistent blocks for K-split launches with K > 6144 (tuning hook)
int g_long_ku = 5;           // K units per wave allowed for rows longer than 12 units (tuning hook: 3 -> 8 waves split K)

template <int M, bool DUAL, int KSPLIT, int KU, int RW, int WQ>   // WQ: 0 bf16, 1 fp8, 2 NF4 (RW == 4), 3 MXFP4 (RW == 4)
__global__ __launch_bounds__(KSPLIT == 1 ? 512 : 64 * KSPLIT) void gemv_stream_kernel(const vv_lin_args a, const int n_groups, const int tune_opt) {
  constexpr bool mx = WQ == 3;
  const int opt = mx ? MX_OPT : tune_opt;            // MXFP4: the fixed policy above, the argument is never read
  constexpr int NW = (KSPLIT == 1) ? 8 : KSPLIT;     // waves per block (KSPLIT == 1: at most; the launcher picks 3 .. 8 so that the row groups divide evenly)
  __shared__ float red[NW * M];
  __shared__ float part[2][NW][RW * M * 2];
  __shared__ __attribute__((aligned(16))) float xs[KSPLIT == 1 ? M * KU * 512 : 4];   // block-staged prologue result (KSPLIT == 1)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwv = (KSPLIT == 1) ? (int)(blockDim.x >> 6) : KSPLIT;
  const int K = a.k, N = a.n, mr = a.m;          // mr <= M real rows
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);
  const bf16_t* __restrict__ W2 = reinterpret_cast<const bf16_t*>(a.w2);
  const unsigned char* __restrict__ C1 = reinterpret_cast<const unsigned char*>(a.w);         // MXFP4: codes and scale bytes
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
  const bool reused = (a.flags & VV_LIN_W_REUSED) != 0 || (opt & 16);    // opt bit 4 (tuning): every matrix with cacheable loads
  constexpr bool f8 = WQ == 1;                   // weight-only fp8 / NF4 are instantiations of their own: the bf16 kernels carry none of it
  constexpr bool nf4 = WQ == 2;
  static_assert(!(nf4 || mx) || (RW == 4 && M <= 2), "NF4, MXFP4: 4 rows per 16-byte code load, decode rows only");
  const int units_k = (K + 511) >> 9;            // NF4, MXFP4: 512-wide units per row in the packed layout
  // the first row group's weight loads are issued before the activation prologue so both latencies overlap
  const int gstride = (KSPLIT == 1) ? gridDim.x * nwv : gridDim.x;
  int g = (KSPLIT == 1) ? blockIdx.x * nwv + wave : blockIdx.x;
  // MXFP4: slot 0 holds the four rows' codes, and a unit's scale dword (byte r = row r) travels beside them in a register of its own (as a lane
  // of a 16-byte slot it pinned all four registers of the slot in both buffers); the other formats never touch the scale arrays
  constexpr int NB = mx ? 1 : RW, NB2 = (DUAL && !mx) ? RW : 1;     // 16-byte slots per unit in a buffer
  constexpr int NS = mx ? KU : 1, NS2 = (mx && DUAL) ? KU : 1;
  u32x4 cur[NB][KU], cur2[NB2][KU];
  u32x4 nxt[NB][KU], nxt2[NB2][KU];
  unsigned int ws[NS], ws2[NS2], nws[NS], nws2[NS2];
  auto issue = [&](u32x4 (&b)[NB][KU], u32x4 (&b2)[NB2][KU], unsigned int (&s)[NS], unsigned int (&s2)[NS2], int grp) {
    // a group past the end (the unconditional second issue of a wave that owns a single group) degenerates to one 16-byte
    // line per instruction: every lane reads element 0 of the matrix
    const bool live = grp < n_groups;
    if constexpr (mx) {        // unit u: 16 B of codes (dword r = row r) in b[0][u], the scale dword in s[u]
      // a group past the end and a unit past the row's end read offset 0 of the matrix: always inside it
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const int unit = (KSPLIT == 1) ? u : (wave + NW * u);
        const bool ok = live && unit < units_k;
        const int64_t gu = ok ? (int64_t)grp * units_k + unit : 0;
        const int64_t co = ok ? (gu * 64 + lane) * 16 : 0;
        const int64_t so = ok ? (gu * 16 + (lane >> 2)) * 4 : 0;
        const u32x4* p1 = reinterpret_cast<const u32x4*>(C1 + co);
        const u32x4* p2 = reinterpret_cast<const u32x4*>(C2 + co);
        if (reused) { b[0][u] = *p1; if constexpr (DUAL) b2[0][u] = *p2; }
        else { b[0][u] = __builtin_nontemporal_load(p1); if constexpr (DUAL) b2[0][u] = __builtin_nontemporal_load(p2); }
        s[u] = *reinterpret_cast<const unsigned int*>(S1 + so);
        if constexpr (DUAL) s2[u] = *reinterpret_cast<const unsigned int*>(S2 + so);
      }
    } else {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int n = min(grp * RW + r, N - 1);
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        if constexpr (nf4) {     // r == 0: this lane's 16 B of codes (4 rows); r == 1, u < (KU + 1) / 2: the scale dword of unit pair u
          const int uu = (r == 0) ? u : 2 * u + (lane >> 5);
          const int unit = (KSPLIT == 1) ? uu : (wave + NW * uu);
          const bool ok = live && uu < KU && unit < units_k;
          if (r == 0) {
            const int64_t co = ok ? (((int64_t)grp * units_k + unit) * 64 + lane) * 16 : 0;
            const u32x4* p1 = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(a.w) + co);
            const u32x4* p2 = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(a.w2) + co);
            if (reused) { b[0][u] = *p1; if (DUAL) b2[0][u] = *p2; }
            else { b[0][u] = __builtin_nontemporal_load(p1); if (DUAL) b2[0][u] = __builtin_nontemporal_load(p2); }
          } else if (r == 1 && 2 * u < KU) {
            const int64_t so = ok ? ((int64_t)grp * units_k + unit) * 32 + (lane & 31) : 0;
            b[1][u].x = __float_as_uint(a.wscale[so]);
            if constexpr (DUAL) b2[1][u].x = __float_as_uint(a.w2scale[so]);
          }
          continue;
        }
        const int64_t off = live ? (int64_t)n * K + koff[u] : 0;
        if (f8) {                // e4m3fn bytes: this lane's 8 weights are 8 bytes
          const u32x2 t = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(a.w) + off));
          b[r][u].x = t.x; b[r][u].y = t.y;
          if (DUAL) {
            const u32x2 t2 = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned char*>(a.w2) + off));
            b2[r][u].x = t2.x; b2[r][u].y = t2.y;
          }
          continue;
        }
        const u32x4* p1 = reinterpret_cast<const u32x4*>(W + off);
        const u32x4* p2 = reinterpret_cast<const u32x4*>(W2 + off);
        if (reused) {            // weights re-read by the next solver step: leave them in L2 / Infinity Cache
          b[r][u] = *p1;
          if (DUAL) b2[r][u] = *p2;
        } else {                 // streamed once per frame: non-temporal, do not pollute the caches
          b[r][u] = __builtin_nontemporal_load(p1);
          if (DUAL) b2[r][u] = __builtin_nontemporal_load(p2);
        }
      }
    }
    }
  };
  // epilogue: output (r, m) of a row group belongs to lane / thread  r * M + m  (KSPLIT == 1: lane of the wave that owns the
  // group; K split: thread of the block), so activations like GELU run once per output in parallel lanes instead of RW x M
  // times in lane 0, and each owner fetches its own operands one group ahead
  constexpr int NE = 1;
  const bool has_eo = a.bias || a.gate || a.res || (!mx && a.wdt == VV_FP8);
  const int eid = (KSPLIT == 1) ? lane : tid;
  EpiOp<!mx> eo_cur[NE], eo_nxt[NE];
  const int eo_id = eid < RW * M ? eid : 0;       // lanes that own no output fetch output 0's operands: no divergent branch around the loads
  const int eo_r = eo_id / M, eo_m = (eo_id - eo_r * M) < mr ? (eo_id - eo_r * M) : mr - 1;
  auto load_eo = [&](EpiOp<!mx> (&e)[NE], int grp) {
    if (!has_eo) return;
    if (opt & 4) { e[0] = epi_load<!mx>(a, eo_m, min((grp < n_groups ? grp : n_groups - 1) * RW + eo_r, N - 1)); return; }
    if constexpr (!mx) {
      if (grp < n_groups && eid < RW * M) e[0] = epi_load_cond(a, eo_m, min(grp * RW + eo_r, N - 1));
    }
  };
  // (MXFP4 sets and moves its one record without the one-trip loop: the loop form gave its kernels another register assignment than they had
  // as a unit of their own, and dropping the loop does the same to the other formats' - profiles/stream_mx_fold.txt)
  if constexpr (mx) {
    eo_cur[0].b = 0.f; eo_cur[0].g = 1.f; eo_cur[0].r = 0.f; eo_nxt[0] = eo_cur[0];
  } else {
#pragma unroll
    for (int i = 0; i < NE; ++i) { eo_cur[i].b = 0.f; eo_cur[i].g = 1.f; eo_cur[i].r = 0.f; eo_cur[i].s = 1.f; eo_cur[i].s2 = 1.f; eo_nxt[i] = eo_cur[i]; }
  }
  float xr[M][KU][8];
  // Activation side.  BATCHED (the per-frame shapes: M * KU <= 8, no SiLU prologue): every load the prologue needs - x rows, norm
  // weight, adaLN shift / scale - is issued in ONE batch AHEAD of the weight loads.  Loads return in order: these are L2 hits and
  // come back first, so the statistics and the normalisation run while the first two row groups of weights are still in flight.
  // (Issued behind the weights, and unit by unit with a full wait each, the prologue was 6-12 dependent round trips that only
  // started once the first weights had landed: +2 us on every kernel with a prologue, +4 us on the dual one.)
  // the SwiGLU (dual) kernels take the block-staged prologue, the others the per-wave batched one: one fast path per instantiation
  // keeps the register allocation of each kernel at what its own path needs
  // (MXFP4: never block-staged, see MX_OPT)
  constexpr bool CAN_STAGE = KSPLIT == 1 && (DUAL || M == 8) && !mx;    // M = 8 (the T = 8 conv stage): 32 KB of activations per WAVE otherwise
  constexpr bool BATCHED = (M * KU <= 8) && !CAN_STAGE;
  // adaLN-modulated rows on a non-dual kernel (the head's 64-row final linear) keep the legacy path: the batch would pin 96 more registers
  const bool batched = BATCHED && ((a.pro == VV_PRO_RMSNORM && !a.mod_scale && (opt & 1)) || (a.pro == VV_PRO_NONE && (opt & 2)));
  bool staged = false;
  if constexpr (CAN_STAGE) staged = a.pro == VV_PRO_RMSNORM && (opt & 8);
  if (CAN_STAGE && staged) {
    // Prologue ONCE PER BLOCK (KSPLIT == 1, RMSNorm): thread t owns the 4-element chunks t, t + T, ... of every row; x, the norm weight
    // and the adaLN shift / scale chunks are requested first, then the first two row groups of weights; statistics through LDS, the
    // normalised rows land in LDS and every lane picks up its k slices from there.  With the prologue per WAVE every one of ~2000
    // waves pulled x, norm weight and modulation (42 KB for the head's SwiGLU GEMV: 86 MB against 28 MB of weights) through L2 at
    // the moment the weight stream saturates the fabric: the median wave saw its activations 4 us after entry (tools/gemv_lab.cpp).
    const int T = nwv * 64;
    constexpr int NCH = (KU * 128 + 191) / 192;     // 4-element chunks per thread per row (blocks have >= 3 waves)
    const bool has_nw = a.norm_w != nullptr, has_mod = a.mod_scale != nullptr;
    float4 xv[M][NCH], nv[NCH], sv[M][NCH], cv[M][NCH];
    const int nchunks = K >> 2;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ch = tid + c * T;
      const int kk = ch < nchunks ? ch * 4 : 0;
#pragma unroll
      for (int m = 0; m < M; ++m) xv[m][c] = *reinterpret_cast<const float4*>(a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx + kk);
      if (has_nw) nv[c] = *reinterpret_cast<const float4*>(a.norm_w + kk);
      if (has_mod) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const int64_t mo = (int64_t)(m < mr ? m : mr - 1) * a.ld_mod + kk;
          sv[m][c] = *reinterpret_cast<const float4*>(a.mod_shift + mo);
          cv[m][c] = *reinterpret_cast<const float4*>(a.mod_scale + mo);
        }
      }
    }
    load_eo(eo_cur, g);
    issue(cur, cur2, ws, ws2, g);
    load_eo(eo_nxt, g + gstride);
    issue(nxt, nxt2, nws, nws2, g + gstride);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
      for (int m = 0; m < M; ++m) VV_FENCE4(xv[m][c]);
      if (has_nw) VV_FENCE4(nv[c]);
      if (has_mod) {
#pragma unroll
        for (int m = 0; m < M; ++m) { VV_FENCE4(sv[m][c]); VV_FENCE4(cv[m][c]); }
      }
    }
    float ss[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      float s1 = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const float4 v = xv[m][c];
        s1 += (tid + c * T < nchunks) ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
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
      for (int w4 = 0; w4 < nwv; ++w4) tot += red[w4 * M + m];      // fixed order: deterministic
      const float rstd = rsqrtf(tot / (float)K + a.eps);
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int ch = tid + c * T;
        float4 v = xv[m][c];
        v.x *= rstd; v.y *= rstd; v.z *= rstd; v.w *= rstd;
        if (has_nw) { v.x *= nv[c].x; v.y *= nv[c].y; v.z *= nv[c].z; v.w *= nv[c].w; }
        if (has_mod) {
          v.x = v.x * (1.0f + cv[m][c].x) + sv[m][c].x; v.y = v.y * (1.0f + cv[m][c].y) + sv[m][c].y;
          v.z = v.z * (1.0f + cv[m][c].z) + sv[m][c].z; v.w = v.w * (1.0f + cv[m][c].w) + sv[m][c].w;
        }
        if (ch < KU * 128) *reinterpret_cast<float4*>(&xs[(m * KU * 128 + ch) * 4]) = ch < nchunks ? v : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        const float4 p = *reinterpret_cast<const float4*>(&xs[m * KU * 512 + u * 512 + lane * 8]);
        const float4 q = *reinterpret_cast<const float4*>(&xs[m * KU * 512 + u * 512 + lane * 8 + 4]);
        xr[m][u][0] = p.x; xr[m][u][1] = p.y; xr[m][u][2] = p.z; xr[m][u][3] = p.w;
        xr[m][u][4] = q.x; xr[m][u][5] = q.y; xr[m][u][6] = q.z; xr[m][u][7] = q.w;
      }
  } else if (BATCHED && batched) {
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
    // the first two row groups go out unconditionally (a group past the end costs one 16-byte line per load instruction) so that
    // no branch separates them from the loads above, and nothing below is scheduled ahead of them
    load_eo(eo_cur, g);
    issue(cur, cur2, ws, ws2, g);
    load_eo(eo_nxt, g + gstride);
    issue(nxt, nxt2, nws, nws2, g + gstride);
    __builtin_amdgcn_sched_barrier(0);
    // everything the prologue computes with is made opaque HERE, behind the weight loads: hipcc otherwise hoists pieces of the
    // arithmetic (and the waits they need) into the blocks above, in front of the weight issue
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int m = 0; m < M; ++m) { VV_FENCE4(xa[m][u]); VV_FENCE4(xb[m][u]); }
      if (has_nw) { VV_FENCE4(na[u]); VV_FENCE4(nb[u]); }
    }
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
      for (int m = 0; m < M; ++m) ss[m] = vv_wave_sum(ss[m]);   // KSPLIT == 1: every wave holds the whole row
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
  if (g < n_groups) { load_eo(eo_cur, g); issue(cur, cur2, ws, ws2, g); }
  if (g + gstride < n_groups) { load_eo(eo_nxt, g + gstride); issue(nxt, nxt2, nws, nws2, g + gstride); }   // two row groups in flight before the prologue even starts
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
        for (int j = 0; j < 8; ++j) xr[m][u][j] = vv_silu(xr[m][u][j]);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) ss = fmaf(xr[m][u][j], xr[m][u][j], ss);
    }
    if (a.pro == VV_PRO_RMSNORM) {
      ss = vv_wave_sum(ss);                               // KSPLIT == 1: every wave holds the whole row
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
        float nw[8], sh[8], sc[8];
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
          sc[0] = c0.x; sc[1] = c0.y; sc[2] = c0.z; sc[3] = c0.w; sc[4] = c1.x; sc[5] = c1.y; sc[6] = c1.z; sc[7] = c1.w;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = xr[m][u][j] * rstd;
          if (a.norm_w) v *= nw[j];
          if (a.mod_scale) v = v * (1.0f + sc[j]) + sh[j];
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
    // The dot products run on packed fp32 FMAs (v_pk_fma_f32: two lanes of a register pair per instruction): even and odd k of a lane
    // accumulate separately and are added once per row group.  This loop, not the memory system, sets the kernel's pace (its time grows
    // 1.2-1.6 us per activation row, tools/mb_rows.py); half the FMA instructions per weight load is the cheapest cut.
    vf2 pacc[RW][M], pacc2[DUAL ? RW : 1][M];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) { pacc[r][m] = vf2{0.f, 0.f}; if (DUAL) pacc2[r][m] = vf2{0.f, 0.f}; }
    if constexpr (nf4) {
      // per wave: 64 tables (unit half h, row r, block b at index 32 h + 8 r + b) x 16 bf16, one slot per weight stream
      __shared__ __attribute__((aligned(16))) unsigned int lut[NW][DUAL ? 2 : 1][64 * 8];
      const int lb = (lane >> 3) * 8;            // this lane's block within a unit, in dwords of its tables
#pragma unroll
      for (int p = 0; p < (KU + 1) / 2; ++p) {
        nf4_build_lut(__uint_as_float(cur[1][p].x), &lut[wave][0][lane * 8]);
        if constexpr (DUAL) nf4_build_lut(__uint_as_float(cur2[1][p].x), &lut[wave][DUAL ? 1 : 0][lane * 8]);
        __builtin_amdgcn_wave_barrier();         // keeps the reads below the writes; a wave's LDS operations complete in order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int u = 2 * p + h;
          if (u >= KU) break;
#pragma unroll
          for (int r = 0; r < RW; ++r) {
            const unsigned short* t1 = reinterpret_cast<const unsigned short*>(&lut[wave][0][(h * 32 + r * 8) * 8 + lb]);
            const unsigned short* t2 = reinterpret_cast<const unsigned short*>(&lut[wave][DUAL ? 1 : 0][(h * 32 + r * 8) * 8 + lb]);
            const unsigned int c1 = cur[0][u][r], c2 = DUAL ? cur2[0][u][r] : 0u;
            float w[8], w2[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              w[i] = __uint_as_float((unsigned int)t1[(c1 >> (4 * i)) & 15u] << 16);
              if (DUAL) w2[i] = __uint_as_float((unsigned int)t2[(c2 >> (4 * i)) & 15u] << 16);
            }
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
              for (int j = 0; j < 8; j += 2) {
                const vf2 xp = {xr[m][u][j], xr[m][u][j + 1]};
                pacc[r][m] = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, xp, pacc[r][m]);
                if (DUAL) pacc2[r][m] = __builtin_elementwise_fma(vf2{w2[j], w2[j + 1]}, xp, pacc2[r][m]);
              }
            }
          }
        }
        __builtin_amdgcn_wave_barrier();         // the next pair's tables overwrite these only after every read above was issued
      }
    } else if constexpr (mx) {
      // the conversion delivers (k, k + 1) as a register pair, which is the packed FMA's operand as it stands
#pragma unroll
      for (int u = 0; u < KU; ++u) {
#pragma unroll
        for (int r = 0; r < RW; ++r) {
          vf2 w[4], w2[4];
          unpack8_mx(cur[0][u][r], (ws[u] >> (8 * r)) & 0xffu, w);
          if constexpr (DUAL) unpack8_mx(cur2[0][u][r], (ws2[u] >> (8 * r)) & 0xffu, w2);
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
    } else {
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        float w[8], w2[8];
        if (f8) { unpack8_f8(cur[r][u], w); if (DUAL) unpack8_f8(cur2[r][u], w2); }
        else { unpack8(cur[r][u], w); if (DUAL) unpack8(cur2[r][u], w2); }
#pragma unroll
        for (int m = 0; m < M; ++m) {
#pragma unroll
          for (int j = 0; j < 8; j += 2) {
            const vf2 xp = {xr[m][u][j], xr[m][u][j + 1]};
            pacc[r][m] = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, xp, pacc[r][m]);
            if (DUAL) pacc2[r][m] = __builtin_elementwise_fma(vf2{w2[j], w2[j + 1]}, xp, pacc2[r][m]);
          }
        }
      }
    }
    }
    float acc[RW][M], acc2[DUAL ? RW : 1][M];
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int m = 0; m < M; ++m) {
        acc[r][m] = vv_wave_sum(pacc[r][m].x + pacc[r][m].y);
        if (DUAL) acc2[r][m] = vv_wave_sum(pacc2[r][m].x + pacc2[r][m].y);
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
        if (n < N && m < mr) epi_pre<!mx>(a, m, n, v, v2, eo_cur[0]);
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
          epi_pre<!mx>(a, m, n, s, s2, eo_cur[0]);
        }
      }
      parity ^= 1;                                 // ping-pong: one barrier per group is enough
    }
    if constexpr (mx) {
      eo_cur[0] = eo_nxt[0];
    } else {
#pragma unroll
      for (int i = 0; i < NE; ++i) eo_cur[i] = eo_nxt[i];
    }
    if constexpr (mx) {                            // one slot per unit, its scale dword beside it: one loop, unit by unit
#pragma unroll
      for (int u = 0; u < KU; ++u) {
        cur[0][u] = nxt[0][u]; ws[u] = nws[u];
        if constexpr (DUAL) { cur2[0][u] = nxt2[0][u]; ws2[u] = nws2[u]; }
      }
    } else {
#pragma unroll
    for (int r = 0; r < RW; ++r)
#pragma unroll
      for (int u = 0; u < KU; ++u) { cur[r][u] = nxt[r][u]; if (DUAL) cur2[r][u] = nxt2[r][u]; }
    }
    g = gn;
    if (g + gstride < n_groups) { load_eo(eo_nxt, g + gstride); issue(nxt, nxt2, nws, nws2, g + gstride); }   // keep two groups in flight
  }
}

int g_dual_rw = 1;            // weight rows per wave step for the dual (SwiGLU) kernel: 1 keeps 4 waves/SIMD resident
int g_small_rw = 2;           // rows per wave step for narrow non-dual matrices (tuning hook)

// Which (dual, ksplit, ku) forms of the M = 1 / 2 / 4 kernels are built (the pieces of stream_exists below):
// whole rows at 1..5 units, 4 / 8 / 16 waves splitting K at 2..5 units per wave; the dual kernel holds two weight streams, so its K-split forms
// stop at 8 waves and 3 units
constexpr bool stream_built(bool dual, int ksplit, int ku) {
  if (ksplit != 1 && ksplit != 4 && ksplit != 8 && ksplit != 16) return false;
  if (ku < 1 || ku > 5 || (ku == 1 && ksplit != 1)) return false;
  if (dual && (ksplit == 16 || (ksplit != 1 && ku > 3))) return false;
  return true;
}
// NF4: <= 2 rows, <= 8 waves (LDS), the dual kernel at <= 4 units per wave (registers)
constexpr bool stream_built_nf4(int m, bool dual, int ksplit, int ku) { return stream_built(dual, ksplit, ku) && m <= 2 && ksplit <= 8 && !(dual && ku > 4); }
// MXFP4, a rule of its own (not NF4's): <= 2 rows; whole rows at 1..5 units, the SwiGLU kernel (two code streams) at 1..4; 4 waves splitting K at
// 2..5 units per wave, 8 waves at 3..5 (2 units x 8 waves is already served by 4 waves x 4 units); SwiGLU with K split: 2..3 units per wave on 4 or
// 8 waves; never 16 waves
constexpr bool stream_built_mx(int m, bool dual, int ksplit, int ku) {
  if (m != 1 && m != 2) return false;
  if (ksplit == 1) return ku >= 1 && ku <= (dual ? 4 : 5);
  if (ksplit != 4 && ksplit != 8) return false;
  if (dual) return ku == 2 || ku == 3;
  return ku >= (ksplit == 4 ? 2 : 3) && ku <= 5;
}
// 5..8 rows: the fragment is 8 rows x KU x 8 floats, so K is split until KU <= 2 (16 waves x 8 rows does not fit the 128-VGPR budget of a 1024-thread block)
constexpr bool stream_built_m8(int ksplit, int ku, int rw) { return (ksplit == 1 && (ku == 1 || ku == 2) && rw == 1) || ((ksplit == 4 || ksplit == 8) && ku == 2 && rw == 2); }
// Every kernel of this file that exists, as (m, dual, ksplit, ku, rw, wq): the launch ladder instantiates under this predicate and nothing else, and
// the decision checks its finished route against it, so neither can name a kernel the other does not have.
//   m = 8      bf16 only, one weight stream
//   NF4, MXFP4 rw = 4 (four rows per 16-byte code load), and no other weight type has rw = 4
//   bf16, fp8  rw = 1 or 2; fp8 for decode rows (m <= 2) only; rw = 1 for the dual kernels (gemv_dual_rw) and the whole-row ones (gemv_small_rw):
//              a non-dual K-split kernel is always rw = 2
constexpr bool stream_exists(int m, bool dual, int ksplit, int ku, int rw, int wq) {
  if (m == 8) return wq == 0 && !dual && stream_built_m8(ksplit, ku, rw);
  if (m != 1 && m != 2 && m != 4) return false;
  if (wq == 2) return rw == 4 && stream_built_nf4(m, dual, ksplit, ku);
  if (wq == 3) return rw == 4 && stream_built_mx(m, dual, ksplit, ku);
  if (wq != 0 && !(wq == 1 && m <= 2)) return false;
  if (rw != 1 && rw != 2) return false;
  if (rw == 1 && !dual && ksplit != 1) return false;
  return stream_built(dual, ksplit, ku);
}

// persistent grid, sized from measurements on MI355X (tools/mb_gemv.py): ~1.5-2 blocks per CU is the sweet spot for the
// wave-per-row layout (more blocks only add prologue copies and a ragged last round), one block per row group when the
// block's waves split K
void stream_grid(const vv_lin_args& a, vv_stream_route& r) {
  const int RW = r.rw, KSPLIT = r.ksplit;
  const bool DUAL = r.dual != 0;
  const int n_groups = (a.n + RW - 1) / RW;
  const int waves = (KSPLIT == 1 && g_waves_override >= 3 && g_waves_override <= 8) ? g_waves_override : 4;
  const int work = (KSPLIT == 1) ? (n_groups + waves - 1) / waves : n_groups;       // blocks if each wave did exactly one group
  // K split: every block reads all of x (M x K fp32 from L2); beyond ~6K columns that traffic rivals the weights, so long
  // rows use fewer, persistent blocks (n=1536 k=8960: 10.4 us at 768 blocks, 9.1 us at 512)
  // (whole rows, dual: 448 at two and four rows per step - bf16 / fp8 under gemv_dual_rw = 2, NF4 - except MXFP4, whose every whole-row cap is 512)
  const int cap = (KSPLIT == 1) ? (DUAL ? ((RW == 1 || r.wq == 3) ? 512 : 448) : 512) : (a.k > 6144 ? g_long_cap : 1024);
  int blocks = work < cap ? work : cap;
  if (g_blocks_override > 0) blocks = g_blocks_override < work ? g_blocks_override : work;
  r.n_groups = n_groups;
  r.blocks = blocks;
  r.threads = KSPLIT == 1 ? 64 * waves : 64 * KSPLIT;
}

// The launch ladder: one run-time switch per template argument, and at its foot the only place a kernel is instantiated - under stream_exists, so
// what is compiled is what can be launched.  A route outside the predicate is declined (false), never served by a neighbouring kernel on a grid
// sized for another rw.
template <int M, bool DUAL, int KSPLIT, int KU, int RW, int WQ>
bool launch_one(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  if constexpr (stream_exists(M, DUAL, KSPLIT, KU, RW, WQ)) {
    hipLaunchKernelGGL((gemv_stream_kernel<M, DUAL, KSPLIT, KU, RW, WQ>), dim3(r.blocks), dim3(r.threads), 0, s, a, r.n_groups, g_opt);
    return true;
  } else {
    return false;
  }
}

template <int M, bool DUAL, int KSPLIT, int KU, int RW>
bool launch_wq(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  switch (r.wq) {
    case 0: return launch_one<M, DUAL, KSPLIT, KU, RW, 0>(a, r, s);
    case 1: return launch_one<M, DUAL, KSPLIT, KU, RW, 1>(a, r, s);
    case 2: return launch_one<M, DUAL, KSPLIT, KU, RW, 2>(a, r, s);   // never a bf16 read of codes
    case 3: return launch_one<M, DUAL, KSPLIT, KU, RW, 3>(a, r, s);
  }
  return false;
}

template <int M, bool DUAL, int KSPLIT, int KU>
bool launch_rw(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  switch (r.rw) {
    case 1: return launch_wq<M, DUAL, KSPLIT, KU, 1>(a, r, s);
    case 2: return launch_wq<M, DUAL, KSPLIT, KU, 2>(a, r, s);
    case 4: return launch_wq<M, DUAL, KSPLIT, KU, 4>(a, r, s);
  }
  return false;
}

template <int M, bool DUAL, int KSPLIT>
bool launch_kus(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  switch (r.ku) {
    case 1: return launch_rw<M, DUAL, KSPLIT, 1>(a, r, s);
    case 2: return launch_rw<M, DUAL, KSPLIT, 2>(a, r, s);
    case 3: return launch_rw<M, DUAL, KSPLIT, 3>(a, r, s);
    case 4: return launch_rw<M, DUAL, KSPLIT, 4>(a, r, s);
    case 5: return launch_rw<M, DUAL, KSPLIT, 5>(a, r, s);
  }
  return false;
}

template <int M, bool DUAL>
bool launch_ku(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  switch (r.ksplit) {
    case 1: return launch_kus<M, DUAL, 1>(a, r, s);
    case 4: return launch_kus<M, DUAL, 4>(a, r, s);
    case 8: return launch_kus<M, DUAL, 8>(a, r, s);
    case 16: return launch_kus<M, DUAL, 16>(a, r, s);
  }
  return false;
}

template <int M>
bool launch_m(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  return r.dual ? launch_ku<M, true>(a, r, s) : launch_ku<M, false>(a, r, s);
}

}  // namespace

void vv_gemv_stream_set_blocks(int b) { g_blocks_override = b; }
void vv_gemv_stream_set_waves(int w) { g_waves_override = w; }
void vv_gemv_stream_set_opt(int o) { g_opt = o; }
void vv_gemv_stream_set_long(int cap, int ku) { if (cap > 0) g_long_cap = cap; if (ku > 0) g_long_ku = ku; }
void vv_gemv_stream_set_dual_rw(int r) { g_dual_rw = r; }
void vv_gemv_stream_set_small_rw(int r) { g_small_rw = r; }

// The one copy of what a call on this unit's weight-only formats must be (vv_common.h): decode rows, whole blocks, scales for every matrix, codes
// and scales aligned for the format's loads, row-major, fp32 in and out.  The activations' alignment and the reach in K stay with the decision.
const char* vv_gemv_stream_refusal(const vv_lin_args& a, int* rc) {
  const bool handoff = (a.flags & (VV_LIN_X_BF16 | VV_LIN_OUT_BF16)) != 0, scales = a.wscale && (!a.w2 || a.w2scale);
  const auto aligned = [&](const void* p, const void* p2, int al) { return (uintptr_t)p % al == 0 && (!a.w2 || (uintptr_t)p2 % al == 0); };
  if (a.wdt == VV_FP8) {        // e4m3fn codes, one fp32 scale per output row
    if (handoff) { if (rc) *rc = VV_E_ARG; return "fp32 activations and outputs (the bf16 hand-off is for bf16 weights)"; }
    if (a.m > 2) return "m <= 2 (3..8 rows read the fragment-major copy, VV_LIN_W_FRAG)";
    if (a.k % 8) return "k % 8 == 0";
    if (!scales) return "row scales for w (and w2)";
    if (!aligned(a.w, a.w2, 8)) return "8-byte aligned rows";
    return nullptr;
  }
  if (a.wdt != VV_NF4 && a.wdt != VV_MXFP4) return "VV_FP8, VV_NF4 or VV_MXFP4 weights";
  const bool nf4 = a.wdt == VV_NF4;      // NF4: 64-blocks, fp32 absmax; MXFP4: 32-blocks, E8M0 scale bytes read 16 at a time
  if (handoff || (a.flags & VV_LIN_W_FRAG)) return "no VV_LIN_W_FRAG and no bf16 hand-off";
  if (a.m < 1 || a.m > 2) return "m <= 2";
  if (nf4 ? a.k % 64 : a.k % 32) return nf4 ? "k % 64 == 0" : "k % 32 == 0";
  if (!scales) return nf4 ? "block scales for w (and w2)" : "scale bytes for w (and w2)";
  if (!aligned(a.w, a.w2, 16)) return "16-byte aligned codes";
  if (!aligned(a.wscale, a.w2scale, nf4 ? 4 : 16)) return nf4 ? "4-byte aligned block scales" : "16-byte aligned scale bytes";
  return nullptr;
}

// The decision: which kernel of this file (or which hot kernel) the call takes, and on what grid.  kind 0 = the shape / alignment is not covered
// (the caller falls back; MXFP4 reaches 40 units of 512, SwiGLU 24).  Reads the arguments' values and alignments and the tune state only.
vv_stream_route vv_gemv_stream_decide(const vv_lin_args& a) {
  vv_stream_route r = {};
  if (a.wdt == VV_BF16 ? (a.m > 8 || a.k % 8) : vv_gemv_stream_refusal(a, nullptr) != nullptr) return r;
  r.wq = a.wdt == VV_MXFP4 ? 3 : a.wdt == VV_NF4 ? 2 : a.wdt == VV_FP8 ? 1 : 0;
  if (a.m > 4) {
    if (a.w2 || a.wdt != VV_BF16) return r;
    if ((uintptr_t)a.w % 16 || (uintptr_t)a.x % 16 || a.ldx % 4) return r;
    if (a.norm_w && (uintptr_t)a.norm_w % 16) return r;
    if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return r;
    const int units8 = (a.k + 511) / 512;
    int ks = 0, ku8 = 0;
    for (int w : {1, 4, 8}) {
      if ((units8 + w - 1) / w <= 2) { ks = w; ku8 = (units8 + w - 1) / w; break; }
    }
    if (!ks) return r;
    if (ks > 1) ku8 = 2;
    r.m = 8; r.ksplit = ks; r.ku = ku8; r.rw = ks == 1 ? 1 : 2;
    if (!stream_exists(r.m, r.dual, r.ksplit, r.ku, r.rw, r.wq)) return r;
    stream_grid(a, r);
    r.kind = VV_GEMV_STREAM;
    return r;
  }
  if (a.wdt == VV_BF16 && ((uintptr_t)a.w % 16 || (a.w2 && (uintptr_t)a.w2 % 16))) return r;
  if ((uintptr_t)a.x % 16) return r;
  if (a.m > 1 && a.ldx % 4) return r;
  if (a.norm_w && (uintptr_t)a.norm_w % 16) return r;
  if (a.mod_scale && ((uintptr_t)a.mod_scale % 16 || (uintptr_t)a.mod_shift % 16 || a.ld_mod % 4)) return r;
  if (a.m == 2 && a.wdt == VV_BF16) {            // the six hot 1.5B shapes: their own kernels (vv_gemv_hot.hip)
    const int id = vv_gemv_hot_covers(a);
    if (id >= 0) { r.kind = VV_GEMV_HOT; r.idx = id; return r; }
  }
  if (a.m == 1 && a.wdt == VV_BF16) {            // the conv tokenizers' one-row W2 and hand-over GEMVs (vv_conv_hot.hip)
    const int id = vv_conv_hot_gemv_covers(a);
    if (id >= 0) { r.kind = VV_GEMV_CONV_HOT; r.idx = id; return r; }
  }
  const int units = (a.k + 511) / 512;
  const bool dual = a.w2 != nullptr;
  // smallest wave count whose per-wave slice fits the register-resident activation fragment (KU <= 5 units; <= 3 for the
  // dual kernel when K is split, its registers hold two weight streams)
  int ksplit = 1, ku = units;
  if (units > ((r.wq >= 2 && dual) ? 4 : 5)) {   // the NF4 SwiGLU kernel holds two code streams and their tables, the MXFP4 one two code streams: <= 4 units
    const int kumax = dual ? 3 : (units > 12 ? g_long_ku : 5);
    ksplit = 0;
    for (int w : {4, 8, 16}) {
      if ((units + w - 1) / w <= kumax) { ksplit = w; ku = (units + w - 1) / w; break; }
    }
    if (!ksplit) return r;
    if (ku < 2) ku = 2;
  }
  r.m = a.m == 1 ? 1 : a.m == 2 ? 2 : 4;
  r.dual = dual; r.ksplit = ksplit; r.ku = ku;
  if (r.wq >= 2) r.rw = 4;                       // NF4, MXFP4: 4 rows per 16-byte code load
  else if (dual) r.rw = g_dual_rw == 1 ? 1 : 2;
  else r.rw = (ksplit == 1 && a.n <= 4096 && g_small_rw == 1) ? 1 : 2;
  if (!stream_exists(r.m, dual, ksplit, ku, r.rw, r.wq)) return r;   // no such kernel (NF4: 16 waves of table slots would not fit the block's LDS; MXFP4 has no 16-wave form)
  stream_grid(a, r);
  r.kind = VV_GEMV_STREAM;
  return r;
}

int vv_launch_gemv_stream_route(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s) {
  if (r.kind == VV_GEMV_HOT) return vv_launch_gemv_hot(a, r.idx, s);
  if (r.kind == VV_GEMV_CONV_HOT) return vv_launch_conv_hot_gemv(a, r.idx, s);
  if (r.kind != VV_GEMV_STREAM) return 0;
  switch (r.m) {
    case 1: return launch_m<1>(a, r, s);
    case 2: return launch_m<2>(a, r, s);
    case 4: return launch_m<4>(a, r, s);
    case 8: return launch_m<8>(a, r, s);   // 5..8 activation rows (the conv tokenizers' T = 8 stage, C = 1024): one pass over the weights instead of two 4-row passes
  }
  return 0;
}

// the names vv_linear_route reports for this file's routes: spelled here and nowhere else
int vv_gemv_stream_route_name(const vv_stream_route& r, char* name, int cap) {
  if (r.kind == VV_GEMV_HOT) return snprintf(name, (size_t)cap, "gemv_hot<%d>", r.idx);
  if (r.kind == VV_GEMV_CONV_HOT) return snprintf(name, (size_t)cap, "conv_hot_gemv<%d>", r.idx);
  if (r.wq == 3) return snprintf(name, (size_t)cap, "gemv_mx<m=%d,dual=%d,ksplit=%d,ku=%d>", r.m, r.dual, r.ksplit, r.ku);   // the MXFP4 routes' documented name (vv_hip.h)
  return snprintf(name, (size_t)cap, "gemv_stream<m=%d,dual=%d,ksplit=%d,ku=%d,rw=%d,wq=%s>", r.m, r.dual, r.ksplit, r.ku, r.rw,
                  r.wq == 2 ? "nf4" : r.wq == 1 ? "fp8" : "bf16");
}

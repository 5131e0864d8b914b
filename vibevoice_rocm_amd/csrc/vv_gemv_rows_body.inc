// vv_gemv_rows_body.inc - the body of gemv_rows_kernel (RT = 1 row tile, 3 .. 8 rows) and gemv_rows16_kernel (RT = 2, 9 .. 16 rows), included by both
// in vv_gemv_rows.hip, which describes it, and of gemv_rows_mx6_kernel (vv_gemv_rows_mx6.hip: WF_MXFP6, RT = 1).  The includer provides DUAL, NW, KS, PERS, WF, RT and the kernel arguments `a` (vv_lin_args) and `x`
// (RowsAux).  Included text, not a device function template: behind a call the 8-row kernels come out with another register allocation.
  constexpr bool F8 = WF == WF_FP8, MX6 = WF == WF_MXFP6, MX = WF == WF_MXFP4 || MX6;      // MX: 128-wide loads, a scale dword beside each (both MX formats)
  constexpr int T = NW * 64;
  static_assert(RT == 1 || (RT == 2 && WF == WF_BF16), "two row tiles: the bf16 form only");
  constexpr int MR = 8 * RT;                        // activation rows
  constexpr int ET = 128 * RT;                      // epilogue threads: one output of a row group each
  constexpr int MS = MAXSPLIT / RT;                 // K slices at most: the partials workspace bound does not depend on RT
  constexpr int FPL = rows_fpl(WF);
  constexpr int KA = FPL * KS;                      // 32-wide A fragments per wave
  constexpr int NCH = (KA + 7) / 8;                 // 4-column chunks per thread per activation row
  constexpr int NM = DUAL ? 2 : 1;
  constexpr int PST = (128 * NM + 8) * RT;          // floats per partial tile: [NM][MR][16] sums + MR partial sums of squares
  constexpr int RW = RT == 1 ? 256 : 128 * RT;      // floats per wave and matrix in `red`
  constexpr bool MOD_OK = NCH == 1;                 // adaLN shift / scale rows: only the instantiations whose slice is one chunk per thread (registers)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  u32x4* xa = reinterpret_cast<u32x4*>(smem);       // [RT][NW][KA][64] A fragments (16 B per lane)
  __shared__ float red[PERS ? 2 : 1][NW][NM][RW];   // per wave: the 16 x 16 accumulator tile(s) (RT > 1: hi + lo rows added); ping-pong when the block walks row groups
  __shared__ float ssr[NW][MR];
  __shared__ float s_tot[MR];
  __shared__ int s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = lane & 15, c = lane >> 4;
  const int ks = blockIdx.y;
  const int K = a.k, N = a.n, mr = a.m;
  const int spw = x.spw, ksplit = x.ksplit, n_groups = x.n_groups;
  const int dbg = MX ? 0 : x.dbg;
  const int spa = FPL * spw;                        // 32-wide k steps per wave
  const int wsteps_total = K >> (MX ? 7 : F8 ? 6 : 5);
  const int step0 = ks * NW * spa;                  // first 32-wide k step of this block
  const int k0 = step0 << 5;
  const bool rms = a.pro == VV_PRO_RMSNORM;
  const bool has_nw = rms && a.norm_w != nullptr, has_mod = MOD_OK && a.mod_scale != nullptr;
  const bool frag = MX || (a.flags & VV_LIN_W_FRAG) != 0;
  const bool reused = (a.flags & VV_LIN_W_REUSED) != 0;

  // ---- requests, oldest first: activations, norm weight, modulation, epilogue operands, then the weights ----------------------------------
  float4 xv[MR][NCH], nv[NCH], sv[8][MOD_OK ? NCH : 1], cv[8][MOD_OK ? NCH : 1];
  bool cval[NCH];
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    const int q = tid + cc * T;
    cval[cc] = q < NW * spa * 8 && (k0 + 4 * q) < K;
    const int kk = (cval[cc] && !(dbg & 4)) ? k0 + 4 * q : 4 * (tid & 7);
#pragma unroll
    for (int m = 0; m < MR; ++m) xv[m][cc] = *reinterpret_cast<const float4*>(a.x + (int64_t)(m < mr ? m : mr - 1) * a.ldx + kk);
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
  // epilogue operands of output (em, en) of a row group = thread tid < ET; absent operands read x[0] (a valid address), ignored at use
  const int em = (tid >> 4) & (MR - 1), en = tid & 15;
  const int emr = em < mr ? em : mr - 1;
  auto load_eo = [&](int grp) {
    int egn = min(grp, n_groups - 1) * 16 + en;
    if constexpr (!MX) egn = min(egn, N - 1);       // MXFP4, MXFP6: N % 16 == 0, in bounds as it is
    EpiOp<false> e;
    const float* pb = a.bias ? a.bias + egn : a.x;
    const float* pg = a.gate ? a.gate + (a.gate_ld ? (int64_t)emr * a.gate_ld + egn : (int64_t)egn) : a.x;
    const float* pr = a.res ? a.res + (int64_t)emr * a.ldres + egn : a.x;
    e.b = *pb; e.g = *pg; e.r = *pr;
    return e;
  };
  const int sb = step0 + wave * spa;                // this wave's first 32-wide k step
  const int sbw = MX ? ks * NW * spw + wave * spw : F8 ? sb >> 1 : sb;      // ... and its first weight load
  const bf16_t* __restrict__ W = reinterpret_cast<const bf16_t*>(a.w);
  const bf16_t* __restrict__ W2 = reinterpret_cast<const bf16_t*>(a.w2);
  const unsigned char* __restrict__ WB = reinterpret_cast<const unsigned char*>(a.w);          // MXFP4: codes and scale bytes
  const unsigned char* __restrict__ WB2 = reinterpret_cast<const unsigned char*>(a.w2);
  const unsigned char* __restrict__ S = reinterpret_cast<const unsigned char*>(a.wscale);
  const unsigned char* __restrict__ S2 = reinterpret_cast<const unsigned char*>(a.w2scale);
  // fp8: the row scale of this lane's weight row (n) in row group grp; N % 16 == 0, so the clamped group is in bounds
  auto wscale_of = [&](const float* sc, int grp) { return F8 ? sc[min(grp, n_groups - 1) * 16 + n] : 1.0f; };
  // a load that is not live (past the row's end, past the last row group, j >= spw) reads the first load of the matrix: a valid address
  // MXFP6: wb / wb2 take the blocks' bytes 16 .. 23 (plane B, behind the N K / 2 bytes of plane A)
  auto issue = [&](u32x4 (&w)[KS], unsigned (&e)[MX ? KS : 1], u32x4 (&w2)[DUAL ? KS : 1], unsigned (&e2)[(MX && DUAL) ? KS : 1],
                   u32x2 (&wb)[MX6 ? KS : 1], u32x2 (&wb2)[(MX6 && DUAL) ? KS : 1], int grp) {
    const bool glive = grp < n_groups;
    int64_t base = 0;                               // in bf16 elements (fp8: two codes per element)
    if constexpr (!MX) {
      if (frag) base = ((int64_t)grp * wsteps_total) * 512 + lane * 8;
      else base = (int64_t)min(grp * 16 + n, N - 1) * K + c * 8;
    }
    const int64_t sstep = frag ? 512 : 32;
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const bool live = glive && j < spw && sbw + j < wsteps_total;
      const u32x4 *p1, *p2;
      const unsigned *q1 = nullptr, *q2 = nullptr;  // MXFP4: the load's scale dword, 4 bytes per weight row
      if constexpr (MX) {
        const int64_t ld = live ? (int64_t)grp * wsteps_total + (sbw + j) : 0;
        p1 = reinterpret_cast<const u32x4*>(WB + (ld * 64 + lane) * 16);
        q1 = reinterpret_cast<const unsigned*>(S + (ld * 16 + n) * 4);
        p2 = reinterpret_cast<const u32x4*>(WB2 + (ld * 64 + lane) * 16);
        q2 = reinterpret_cast<const unsigned*>(S2 + (ld * 16 + n) * 4);
        if constexpr (MX6) {
          const int64_t pb = (int64_t)N * K / 2 + (ld * 64 + lane) * 8;
          const u32x2 *r1 = reinterpret_cast<const u32x2*>(WB + pb), *r2 = reinterpret_cast<const u32x2*>(WB2 + pb);
          if (reused) { wb[j] = *r1; if (DUAL) wb2[j] = *r2; }
          else { wb[j] = __builtin_nontemporal_load(r1); if (DUAL) wb2[j] = __builtin_nontemporal_load(r2); }
        }
      } else {
        const int64_t off = live ? base + (int64_t)(sbw + j) * sstep : 0;
        p1 = reinterpret_cast<const u32x4*>(W + off);
        p2 = reinterpret_cast<const u32x4*>(W2 + off);
      }
      if (reused) {
        w[j] = *p1;
        if constexpr (MX) e[j] = *q1;
        if (DUAL) { w2[j] = *p2; if constexpr (MX) e2[j] = *q2; }
      } else {
        w[j] = __builtin_nontemporal_load(p1);
        if constexpr (MX) e[j] = __builtin_nontemporal_load(q1);
        if (DUAL) { w2[j] = __builtin_nontemporal_load(p2); if constexpr (MX) e2[j] = __builtin_nontemporal_load(q2); }
      }
    }
  };
  const int gstride = gridDim.x;
  int g = blockIdx.x;
  u32x4 wc[KS], wc2[DUAL ? KS : 1];
  u32x4 wn[PERS ? KS : 1], wn2[(PERS && DUAL) ? KS : 1];
  unsigned ec[MX ? KS : 1], ec2[(MX && DUAL) ? KS : 1];                       // MXFP4: the loads' scale dwords
  unsigned en_[(MX && PERS) ? KS : 1], en2[(MX && PERS && DUAL) ? KS : 1];
  u32x2 bc[MX6 ? KS : 1], bc2[(MX6 && DUAL) ? KS : 1], bn[(MX6 && PERS) ? KS : 1], bn2[(MX6 && PERS && DUAL) ? KS : 1];      // MXFP6: plane B
  EpiOp<false> eo = load_eo(g), eo_n = eo;
  float sc = 1.0f, sc2 = 1.0f, sn = 1.0f, sn2 = 1.0f;                         // fp8: the row scales
  if constexpr (F8) { sc = wscale_of(a.wscale, g); if (DUAL) sc2 = wscale_of(a.w2scale, g); }
  issue(wc, ec, wc2, ec2, bc, bc2, g);
  if constexpr (PERS && RT == 1) {
    eo_n = load_eo(g + gstride);
    if constexpr (F8) { sn = wscale_of(a.wscale, g + gstride); if (DUAL) sn2 = wscale_of(a.w2scale, g + gstride); }
    issue(wn, en_, wn2, en2, bn, bn2, g + gstride);
  }
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
#pragma unroll
    for (int m = 0; m < MR; ++m) VV_FENCE4(xv[m][cc]);
    if (has_nw) VV_FENCE4(nv[cc]);
    if constexpr (MOD_OK) {
      if (has_mod) {
#pragma unroll
        for (int m = 0; m < 8; ++m) { VV_FENCE4(sv[m][cc]); VV_FENCE4(cv[m][cc]); }
      }
    }
  }

  // ---- activation prologue -------------------------------------------------------------------------------------------------------------
  float rstd[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) rstd[m] = 1.0f;
  if (rms) {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
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
    if (tid < MR) {
      float tot = 0.f;
#pragma unroll
      for (int w4 = 0; w4 < NW; ++w4) tot += ssr[w4][tid];          // fixed order: deterministic
      s_tot[tid] = tot;
    }
    __syncthreads();
    if (ksplit == 1) {
#pragma unroll
      for (int m = 0; m < MR; ++m) rstd[m] = rsqrtf(s_tot[m] / (float)K + a.eps);
    }
  }
#pragma unroll
  for (int cc = 0; cc < NCH; ++cc) {
    const int q = tid + cc * T;
    if (q >= NW * KA * 8) continue;
    const int js = q >> 3, wv = js / spa, jk = js - wv * spa;       // block-relative k step -> (wave, step of the wave)
    if (wv >= NW) continue;
    // MXFP6: MFMA h of a load meets elements 8 h .. 8 h + 7 of the block of lane quarter c, k = 128 J + 32 c + 8 h + i: the 8-wide piece that
    // is quarter cq of step 4 J + h in k order goes to quarter h of fragment 4 J + cq
    const int j = MX6 ? (jk & ~3) | ((q & 7) >> 1) : jk;
    const int cq = MX6 ? jk & 3 : (q & 7) >> 1, half = q & 1;
    {
      constexpr int t = 0;
#include "vv_gemv_rows_tile.inc"
    }
    if constexpr (RT == 2) {
      constexpr int t = 1;
#include "vv_gemv_rows_tile.inc"
    }
  }
  if constexpr (PERS && RT == 2) {                  // two tiles: the next row group's weights are requested here, once the prologue's registers are free
    eo_n = load_eo(g + gstride);
    issue(wn, en_, wn2, en2, bn, bn2, g + gstride);
  }
  __syncthreads();
  u32x4 af[RT][KA];
#pragma unroll
  for (int j = 0; j < KA; ++j) {
    af[0][j] = xa[(wave * KA + j) * 64 + lane];
    if constexpr (RT == 2) af[1][j] = xa[(wave * KA + j) * 64 + lane + NW * KA * 64];
  }

  // ---- the weights meet the fragments: one row group per pass -------------------------------------------------------------------------
  int pp_ = 0;
  while (g < n_groups) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
    f32x4 acch, acc2h;                  // RT == 2: the second row tile's (set there only: a dead initialisation changes the 8-row kernels' register allocation)
    if constexpr (RT == 2) { acch = f32x4{0.f, 0.f, 0.f, 0.f}; acc2h = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      if (j < spw && sbw + j < wsteps_total) {
        if constexpr (F8) {              // the two 32-wide halves in k order: the summation order of the bf16 kernel
          bf16x8 b0, b1;
          fp8_frags(wc[j], sc, b0, b1);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][2 * j]), b0, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][2 * j + 1]), b1, acc, 0, 0, 0);
          if (DUAL) {
            fp8_frags(wc2[j], sc2, b0, b1);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][2 * j]), b0, acc2, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][2 * j + 1]), b1, acc2, 0, 0, 0);
          }
        } else if constexpr (MX6) {      // the lane's whole block decoded at once; MFMA h takes its elements 8 h .. 8 h + 7 (the fragments' k order above)
          const bf16x32 b = mx6_block(wc[j], bc[j], (ec[j] >> (8 * c)) & 0xffu);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 0]), __builtin_shufflevector(b, b, 0, 1, 2, 3, 4, 5, 6, 7), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 1]), __builtin_shufflevector(b, b, 8, 9, 10, 11, 12, 13, 14, 15), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 2]), __builtin_shufflevector(b, b, 16, 17, 18, 19, 20, 21, 22, 23), acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 3]), __builtin_shufflevector(b, b, 24, 25, 26, 27, 28, 29, 30, 31), acc, 0, 0, 0);
          if (DUAL) {
            const bf16x32 b2 = mx6_block(wc2[j], bc2[j], (ec2[j] >> (8 * c)) & 0xffu);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 0]), __builtin_shufflevector(b2, b2, 0, 1, 2, 3, 4, 5, 6, 7), acc2, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 1]), __builtin_shufflevector(b2, b2, 8, 9, 10, 11, 12, 13, 14, 15), acc2, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 2]), __builtin_shufflevector(b2, b2, 16, 17, 18, 19, 20, 21, 22, 23), acc2, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + 3]), __builtin_shufflevector(b2, b2, 24, 25, 26, 27, 28, 29, 30, 31), acc2, 0, 0, 0);
          }
        } else if constexpr (MX) {       // the four 32-wide steps of the load in k order: the summation order of the bf16 kernel
#pragma unroll
          for (int h = 0; h < 4; ++h) {
            const bf16x8 b = mx_frag(wc[j][h], (ec[j] >> (8 * h)) & 0xffu);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + h]), b, acc, 0, 0, 0);
            if (DUAL) {
              const bf16x8 b2 = mx_frag(wc2[j][h], (ec2[j] >> (8 * h)) & 0xffu);
              acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][4 * j + h]), b2, acc2, 0, 0, 0);
            }
          }
        } else {
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][j]), __builtin_bit_cast(bf16x8, wc[j]), acc, 0, 0, 0);
          if (DUAL) acc2 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[0][j]), __builtin_bit_cast(bf16x8, wc2[j]), acc2, 0, 0, 0);
          if constexpr (RT == 2) {       // the same B fragment against the second row tile: the weights are read once for all 16 rows
            acch = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[1][j]), __builtin_bit_cast(bf16x8, wc[j]), acch, 0, 0, 0);
            if (DUAL) acc2h = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[1][j]), __builtin_bit_cast(bf16x8, wc2[j]), acc2h, 0, 0, 0);
          }
        }
      }
    }
    // accumulator: lane (n, c) holds fragment rows 4 c + i of weight row n
    if constexpr (RT == 1) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        red[pp_][wave][0][(4 * c + i) * 16 + n] = acc[i];
        if (DUAL) red[pp_][wave][NM - 1][(4 * c + i) * 16 + n] = acc2[i];
      }
    } else {                             // lanes c and c + 2 hold the high and the low part of the same activation rows: added here, in that order
#pragma unroll
      for (int t = 0; t < RT; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = t ? acch[i] : acc[i], o = __shfl_xor(v, 32);
          if (c < 2) red[pp_][wave][0][t * 128 + (4 * c + i) * 16 + n] = v + o;
          if (DUAL) {
            const float v2 = t ? acc2h[i] : acc2[i], o2 = __shfl_xor(v2, 32);
            if (c < 2) red[pp_][wave][NM - 1][t * 128 + (4 * c + i) * 16 + n] = v2 + o2;
          }
        }
      }
    }
    __syncthreads();
    float s = 0.f, s2 = 0.f;
    if constexpr (RT == 1) {
      if (tid < 128) {
#pragma unroll
        for (int w4 = 0; w4 < NW; ++w4) {
          s += red[pp_][w4][0][tid] + red[pp_][w4][0][tid + 128];               // high-part row + low-part row
          if (DUAL) s2 += red[pp_][w4][NM - 1][tid] + red[pp_][w4][NM - 1][tid + 128];
        }
      }
    } else if (tid < ET) {
#pragma unroll
      for (int w4 = 0; w4 < NW; ++w4) {
        s += red[pp_][w4][0][tid];
        if (DUAL) s2 += red[pp_][w4][NM - 1][tid];
      }
    }
    float rs = 1.0f;
    if (!PERS && ksplit > 1 && x.atomic) {
      if (tid < ET) {
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
    if (!PERS && ksplit > 1 && !(dbg & 2)) {
      // partial tile out (write-through), ticket, the last block of the row group folds
      float* pp = x.part + ((int64_t)g * ksplit + ks) * PST;
      if (tid < ET) {
        __hip_atomic_store(pp + tid, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (DUAL) __hip_atomic_store(pp + ET + tid, s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if (tid < MR) __hip_atomic_store(pp + ET * NM + tid, rms ? s_tot[tid] : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) {
        const int tk = __hip_atomic_fetch_add(&x.tickets[g], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (tk == ksplit - 1);
        if (s_last) __hip_atomic_store(&x.tickets[g], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // ready for the next launch
      }
      __syncthreads();
      if (!s_last) return;
      if (tid >= ET) return;
      const float* p0 = x.part + (int64_t)g * ksplit * PST;
      float pv[MS], pv2[DUAL ? MS : 1], pq[MS];
#pragma unroll
      for (int i = 0; i < MS; ++i) {                                  // every partial requested before the first is used
        const int ii = i < ksplit ? i : 0;
        pv[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (DUAL) pv2[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + ET + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pq[i] = __hip_atomic_load(p0 + (int64_t)ii * PST + ET * NM + em, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      s = 0.f; s2 = 0.f;
      float q2 = 0.f;
#pragma unroll
      for (int i = 0; i < MS; ++i) {
        if (i < ksplit) { s += pv[i]; if (DUAL) s2 += pv2[i]; q2 += pq[i]; }
      }
      if (rms) rs = rsqrtf(q2 / (float)K + a.eps);
    }
    if (tid < ET) {
      const int gn = g * 16 + en;
      // the shared sequence on this thread's output.  The shape is the one that leaves the instruction streams as they were: v assigned in two
      // blocks and the operands handed over by value.  With eo by reference, or v initialised and used in one block, the persistent DUAL
      // kernels come out with the same instructions on other registers (4 .. 8 of the 44; DESIGN.md, "One epilogue, one set of device helpers")
      float v = s * rs, v2 = s2 * rs;
      if (em < mr && gn < N) {
        v = vv_epi_value(a, v, v2, EpiHeld{eo.b, eo.g, eo.r});
        a.out[(int64_t)em * a.ldo + gn] = v;
      }
    }
    if constexpr (!PERS) {
      break;
    } else {
      g += gstride;
      pp_ ^= 1;                                        // ping-pong: one barrier per row group is enough
      eo = eo_n;
      sc = sn; sc2 = sn2;
#pragma unroll
      for (int j = 0; j < KS; ++j) {
        wc[j] = wn[j]; if (DUAL) wc2[j] = wn2[j];
        if constexpr (MX) { ec[j] = en_[j]; if (DUAL) ec2[j] = en2[j]; }
        if constexpr (MX6) { bc[j] = bn[j]; if (DUAL) bc2[j] = bn2[j]; }
      }
      if (g + gstride < n_groups) {
        eo_n = load_eo(g + gstride);
        if constexpr (F8) { sn = wscale_of(a.wscale, g + gstride); if (DUAL) sn2 = wscale_of(a.w2scale, g + gstride); }
        issue(wn, en_, wn2, en2, bn, bn2, g + gstride);
      }
    }
  }

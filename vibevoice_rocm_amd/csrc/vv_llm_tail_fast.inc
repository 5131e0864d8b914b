// body of llm_tail_fast_kernel / llm_tail_fast_rows_kernel (vv_fused.hip): the kernels' parameters, MODE, and - named in every mode, read in
// theirs only - smp, q (TAIL_SAMPLE) and samplers, seeds (TAIL_ROWS) are in scope
  {   // dialogues of a row-batched step: block b owns rows 2 b, 2 b + 1 and the b-th token / forced token / counters
    const int b = blockIdx.x;
    h += (int64_t)2 * b * ldh; out += (int64_t)2 * b * ldo; logits_out += 8 * b; token_out += b;
    if (forced) forced += b;
    if (lens) lens += 2 * b;
    if (frame_ctr) frame_ctr += b;
    if (active) active += b;
    if constexpr (MODE == TAIL_SAMPLE) q += 8 * b;
    if constexpr (MODE == TAIL_ROWS) { samplers += b; seeds += b; }
  }
  constexpr int NC = 4, NV = 8;                    // column chunks (of 4) per thread per row, constrained ids
  __shared__ float red[4][2];
  __shared__ float lgp[4][NV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H4 = H >> 2;
  vv_sampler srow = smp;
  uint64_t seed = 0;
  int pos = 0;
  // TAIL_ROWS: the block's sampler row, token seed and position, requested ahead of the weight rows (they return first: q below waits for them alone)
  if constexpr (MODE == TAIL_ROWS) { srow = *samplers; seed = *seeds; pos = lens[0]; }
  float4 xv[2][NC], nw[NC], wv[NV][NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int ch = tid + 256 * c;
    const int k = ch < H4 ? 4 * ch : 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) xv[r][c] = *reinterpret_cast<const float4*>(h + (int64_t)(r < R ? r : 0) * ldh + k);
    nw[c] = *reinterpret_cast<const float4*>(norm_w + k);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const WT* wr = w_valid + (int64_t)(i < nv ? i : 0) * H + k;
      if constexpr (sizeof(WT) == 2) {
        const uint2 p = *reinterpret_cast<const uint2*>(wr);
        wv[i][c] = make_float4(__uint_as_float(p.x << 16), __uint_as_float(p.x & 0xffff0000u), __uint_as_float(p.y << 16), __uint_as_float(p.y & 0xffff0000u));
      } else {
        wv[i][c] = *reinterpret_cast<const float4*>(wr);
      }
    }
  }
  int idv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) idv[i] = ids[i < nv ? i : 0];
  const int fv = forced ? *forced : -1;
  const int live = active ? *active : 1;
  float qv[NV];
  if constexpr (MODE == TAIL_SAMPLE) {
#pragma unroll
    for (int i = 0; i < NV; ++i) qv[i] = (tid == 0 && i < nv) ? q[i] : 1.f;
  }
  if constexpr (MODE == TAIL_ROWS) {
#pragma unroll
    for (int i = 0; i < NV; ++i) qv[i] = 1.f;
    if (tid == 0) vv_token_draws8(seed, (unsigned)pos, nv, qv);      // two Philox blocks + nv logf in one lane, while the burst above is in flight
  }
  const int l0 = MODE == TAIL_ROWS ? pos : (lens ? lens[0] : 0), l1 = lens ? lens[1] : 0, fc = frame_ctr ? *frame_ctr : 0;
  float ss[2] = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const bool cv = tid + 256 * c < H4;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const float4 v = xv[r][c];
      ss[r] += cv ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
    }
  }
  ss[0] = vv_wave_sum(ss[0]); ss[1] = vv_wave_sum(ss[1]);
  if (lane == 0) { red[wave][0] = ss[0]; red[wave][1] = ss[1]; }
  __syncthreads();
  float lg[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) lg[i] = 0.f;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (r >= R) break;
    const float rstd = rsqrtf(((red[0][r] + red[1][r]) + (red[2][r] + red[3][r])) / (float)H + eps);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int ch = tid + 256 * c;
      if (ch >= H4) continue;
      const float4 v = make_float4(xv[r][c].x * rstd * nw[c].x, xv[r][c].y * rstd * nw[c].y, xv[r][c].z * rstd * nw[c].z, xv[r][c].w * rstd * nw[c].w);
      *reinterpret_cast<float4*>(out + (int64_t)r * ldo + 4 * ch) = v;
      if (r == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) lg[i] += (wv[i][c].x * v.x + wv[i][c].y * v.y) + (wv[i][c].z * v.z + wv[i][c].w * v.w);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float t = vv_wave_sum(lg[i]);
    if (lane == 0) lgp[wave][i] = t;
  }
  __syncthreads();
  if (tid == 0) {
    float l[NV];
    int best = 0;
    for (int i = 0; i < nv; ++i) {
      l[i] = (lgp[0][i] + lgp[1][i]) + (lgp[2][i] + lgp[3][i]);
      logits_out[i] = l[i];
      if (MODE == TAIL_ARGMAX && i && (l[i] > l[best] || (l[i] == l[best] && idv[i] < idv[best]))) best = i;
    }
    if constexpr (MODE == TAIL_SAMPLE) {
      if (fv < 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) if (i >= nv) l[i] = 0.f;
        best = vv_sample_choice(l, nv, smp, qv);
      }
    }
    if constexpr (MODE == TAIL_ROWS) {
      if (fv < 0 && srow.temperature > 0.f) {
#pragma unroll
        for (int i = 0; i < NV; ++i) if (i >= nv) l[i] = 0.f;
        best = vv_sample_choice(l, nv, srow, qv);
      } else if (fv < 0) {                             // a greedy row (temperature 0): the argmax instantiation's rule
        for (int i = 1; i < nv; ++i)
          if (l[i] > l[best] || (l[i] == l[best] && idv[i] < idv[best])) best = i;
      }
    }
    const int t = fv >= 0 ? fv : idv[best];
    *token_out = t;
    if (lens && live) {                              // a finished dialogue of the batch keeps its positions (its rows are computed and dropped)
      lens[0] = l0 + 1;
      if (tok_start < 0) { lens[1] = l1 + 1; if (t == tok_diff && frame_ctr) *frame_ctr = fc + 1; }   // refresh_negative=False: the negative row consumes every token
      else if (t == tok_start) lens[1] = 0;
      else if (t == tok_diff) { lens[1] = l1 + 1; if (frame_ctr) *frame_ctr = fc + 1; }
    }
  }

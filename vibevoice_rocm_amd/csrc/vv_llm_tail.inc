// body of llm_tail_kernel / llm_tail_rows_kernel (vv_fused.hip): the kernels' parameters, MODE, and - named in every mode, read in theirs only -
// smp, q (TAIL_SAMPLE) and samplers, seeds (TAIL_ROWS) are in scope
  extern __shared__ float hn0[];          // [H] normalised row 0 (the positive branch: the only row logits are taken from)
  __shared__ float red[4];
  __shared__ float lg[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  vv_sampler srow = smp;
  float qrow[8];                          // TAIL_ROWS, thread 0: the dialogue's draws at the position lens[0] holds at entry (it is advanced below)
  if constexpr (MODE == TAIL_ROWS) {
    srow = samplers[0];
    if (tid == 0) vv_token_draws8(seeds[0], (unsigned)lens[0], nv, qrow);
  }
  for (int r = 0; r < R; ++r) {
    const float* xr = h + (int64_t)r * ldh;
    float s = 0.f;
    for (int c = tid; c < H; c += 256) { const float v = xr[c]; s = fmaf(v, v, s); }
    s = vv_wave_sum(s);
    __syncthreads();
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const float rstd = rsqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)H + eps);
    for (int c = tid; c < H; c += 256) {
      const float v = xr[c] * rstd * norm_w[c];
      out[(int64_t)r * ldo + c] = v;
      if (r == 0) hn0[c] = v;
    }
  }
  __syncthreads();
  for (int i = wave; i < nv; i += 4) {                // one wave per constrained vocabulary row
    const WT* wr = w_valid + (int64_t)i * H;
    float s = 0.f;
    for (int c = lane; c < H; c += 64) s = fmaf(ldw(wr + c), hn0[c], s);
    s = vv_wave_sum(s);
    if (lane == 0) { lg[i] = s; logits_out[i] = s; }
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    if constexpr (MODE == TAIL_SAMPLE) {
      float l8[8], q8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { l8[i] = i < nv ? lg[i] : 0.f; q8[i] = i < nv ? q[i] : 1.f; }
      best = vv_sample_choice(l8, nv, smp, q8);
    } else if (MODE == TAIL_ROWS && srow.temperature > 0.f) {      // a row that is not > 0 (greedy, or a NaN) takes the argmax below
      float l8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) l8[i] = i < nv ? lg[i] : 0.f;
      best = vv_sample_choice(l8, nv, srow, qrow);
    } else {
    for (int i = 1; i < nv; ++i)
      if (lg[i] > lg[best] || (lg[i] == lg[best] && ids[i] < ids[best])) best = i;     // first maximum in ascending id order, as torch.argmax over the masked vocabulary
    }
    const int f = forced ? *forced : -1;
    const int t = f >= 0 ? f : ids[best];
    *token_out = t;
    if (lens) {
      lens[0] += 1;
      if (tok_start < 0) { lens[1] += 1; if (t == tok_diff && frame_ctr) *frame_ctr += 1; }      // refresh_negative=False: the negative row consumes every token
      else if (t == tok_start) lens[1] = 0;
      else if (t == tok_diff) { lens[1] += 1; if (frame_ctr) *frame_ctr += 1; }
    }
  }

// The body of head_boundary_kernel (vv_fused.hip), included once per kernel that runs it: in scope are the template parameters KU and SDE and
// the kernel's own BoundaryArgs a.  Kept as text, not as a function: the scalar-guidance kernels then compile to exactly the code they had
// before the per-utterance form existed (tools/isa_diff.py).
  {
    const int b = blockIdx.y;
    a.h += 2 * b * a.ldh; a.shift += 2 * b * a.ld_mod; a.scale += 2 * b * a.ld_mod;
    a.Xs += b * a.state_stride; a.Ms += b * a.state_stride; a.h_out += 2 * b * a.ldh_out; a.latent_out += b * a.latent_stride;
    if constexpr (SDE) a.nx += b * a.nx_stride;
  }
  __shared__ __attribute__((aligned(16))) float ys[KU * 512];
  __shared__ float red[4][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = a.D, N = a.D + a.latent;
  constexpr int NCH = (KU * 128 + 255) / 256;
  const int nchunks = D >> 2;
  // activation side first (see gemv_stream_kernel): h rows, shift / scale rows of both branches
  float4 hv[2][NCH], sv[2][NCH], cv[2][NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int ch = tid + c * 256;
    const int kk = ch < nchunks ? ch * 4 : 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      hv[r][c] = *reinterpret_cast<const float4*>(a.h + r * a.ldh + kk);
      sv[r][c] = *reinterpret_cast<const float4*>(a.shift + r * a.ld_mod + kk);
      cv[r][c] = *reinterpret_cast<const float4*>(a.scale + r * a.ld_mod + kk);
    }
  }
  const int gstride = gridDim.x * 4;
  int g = blockIdx.x * 4 + wave;
  float4 cur[KU][2], nxt[KU][2];
  auto issue = [&](float4 (&b)[KU][2], int row) {
    const bool live = row < N;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const int k0 = u * 512 + lane * 8;
      const int64_t off = (live && k0 < D) ? (int64_t)row * D + k0 : 0;
      b[u][0] = *reinterpret_cast<const float4*>(a.G + off);
      b[u][1] = *reinterpret_cast<const float4*>(a.G + off + 4);
    }
  };
  float xs_cur = a.Xs[g < N ? g : 0], ms_cur = a.Ms[g < N ? g : 0];
  float nx_cur = 0.f, nx_nxt = 0.f;
  if constexpr (SDE) nx_cur = a.nx[g < N ? g : 0];
  issue(cur, g);
  float xs_nxt = a.Xs[g + gstride < N ? g + gstride : 0], ms_nxt = a.Ms[g + gstride < N ? g + gstride : 0];
  if constexpr (SDE) nx_nxt = a.nx[g + gstride < N ? g + gstride : 0];
  issue(nxt, g + gstride);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int r = 0; r < 2; ++r) { VV_FENCE4(hv[r][c]); VV_FENCE4(sv[r][c]); VV_FENCE4(cv[r][c]); }
  float ss[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const float4 v = hv[r][c];
      s1 += (tid + c * 256 < nchunks) ? (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w) : 0.f;
    }
    ss[r] = vv_wave_sum(s1);
  }
  if (lane == 0) { red[wave][0] = ss[0]; red[wave][1] = ss[1]; }
  __syncthreads();
  {
    const float rs0 = rsqrtf(((red[0][0] + red[1][0]) + (red[2][0] + red[3][0])) / (float)D + a.eps);
    const float rs1 = rsqrtf(((red[0][1] + red[1][1]) + (red[2][1] + red[3][1])) / (float)D + a.eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int ch = tid + c * 256;
      if (ch < KU * 128) {
        float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ch < nchunks) {
          const float4 h0 = hv[0][c], h1 = hv[1][c];
          // FinalLayer: modulate(norm_final(h), shift, scale) per branch, then classifier-free guidance on the (linear) remainder
          const float yc0 = h0.x * rs0 * (1.0f + cv[0][c].x) + sv[0][c].x, yu0 = h1.x * rs1 * (1.0f + cv[1][c].x) + sv[1][c].x;
          const float yc1 = h0.y * rs0 * (1.0f + cv[0][c].y) + sv[0][c].y, yu1 = h1.y * rs1 * (1.0f + cv[1][c].y) + sv[1][c].y;
          const float yc2 = h0.z * rs0 * (1.0f + cv[0][c].z) + sv[0][c].z, yu2 = h1.z * rs1 * (1.0f + cv[1][c].z) + sv[1][c].z;
          const float yc3 = h0.w * rs0 * (1.0f + cv[0][c].w) + sv[0][c].w, yu3 = h1.w * rs1 * (1.0f + cv[1][c].w) + sv[1][c].w;
          y = make_float4(yu0 + a.cfg * (yc0 - yu0), yu1 + a.cfg * (yc1 - yu1), yu2 + a.cfg * (yc2 - yu2), yu3 + a.cfg * (yc3 - yu3));
        }
        *reinterpret_cast<float4*>(&ys[ch * 4]) = y;
      }
    }
  }
  __syncthreads();
  float yr[KU][8];
#pragma unroll
  for (int u = 0; u < KU; ++u) {
    const float4 p = *reinterpret_cast<const float4*>(&ys[u * 512 + lane * 8]);
    const float4 q = *reinterpret_cast<const float4*>(&ys[u * 512 + lane * 8 + 4]);
    yr[u][0] = p.x; yr[u][1] = p.y; yr[u][2] = p.z; yr[u][3] = p.w; yr[u][4] = q.x; yr[u][5] = q.y; yr[u][6] = q.z; yr[u][7] = q.w;
  }
  while (g < N) {
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      const float w[8] = {cur[u][0].x, cur[u][0].y, cur[u][0].z, cur[u][0].w, cur[u][1].x, cur[u][1].y, cur[u][1].z, cur[u][1].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) acc = fmaf(w[j], yr[u][j], acc);
    }
    const float z = vv_wave_sum(acc);
    if (lane == 0) {
      const float x0 = a.k.alpha_s * xs_cur - a.k.sigma_s * z;
      float xt = a.k.cx * xs_cur - a.k.cd * x0;
      if (a.k.order == 2) xt -= 0.5f * a.k.cd * (a.k.rinv * (x0 - ms_cur));
      if constexpr (SDE) xt = fmaf(a.k.cn, nx_cur, xt);        // variance noise of this step, as vv_dpm_proj adds it to x
      a.Xs[g] = xt;
      a.Ms[g] = x0;
      if (g < D) { a.h_out[g] = xt; a.h_out[a.ldh_out + g] = xt; }
      else a.latent_out[g - D] = xt;
    }
    g += gstride;
#pragma unroll
    for (int u = 0; u < KU; ++u) { cur[u][0] = nxt[u][0]; cur[u][1] = nxt[u][1]; }
    xs_cur = xs_nxt; ms_cur = ms_nxt;
    if constexpr (SDE) nx_cur = nx_nxt;
    if (g + gstride < N) {
      xs_nxt = a.Xs[g + gstride]; ms_nxt = a.Ms[g + gstride];
      if constexpr (SDE) nx_nxt = a.nx[g + gstride];
      issue(nxt, g + gstride);
    }
  }

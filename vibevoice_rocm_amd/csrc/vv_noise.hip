// vv_noise_normal: the diffusion sampler's Gaussian noise drawn on the device (vv_hip.h) - the initial latent of a frame and, for the SDE
// solver, the variance noise of its steps - from a counter-based generator, so that a frame's noise is a pure function of (the dialogue's
// seed, the frame index, the kind of row, the element) and the launch can sit inside the captured frame with nothing uploaded but the index.
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): key = the seed's two halves, counter = (quad, frame,
// kind, 0).  The four 32-bit outputs become uniforms u = x * 2^-32 + 2^-33 in (0, 1] (x * 2^-32 is exact in fp32, so the sum rounds once
// whether or not it is contracted into an fma; x = 2^32 - 1 converts to 2^32 and gives u = 1), and two Box-Muller pairs:
// z[4 j] = r(u0) cos(2 pi u1), z[4 j + 1] = r(u0) sin(2 pi u1), z[4 j + 2], z[4 j + 3] the same from (u2, u3), r(u) = sqrt(-2 log u), with
// the full-precision logf / sinf / cosf (tests/philox_ref.py restates all of it in numpy; the kernel is held to 2e-5 of its fp64 evaluation).
//
// One thread per quad and one launch for every row of the call: B x (1 + n_steps) x ceil(n / 4) threads, 16 per row at latent 64.  The work
// of a thread is ~40 integer multiplies and three libm calls, the whole launch a few waves: its time is the launch itself, so there is
// nothing to tile - 64-thread workgroups spread the quads of an SDE call (B = 4, 20 steps: 1344) over 21 CUs instead of 6.
#include "vv_common.h"

namespace {

// philox4x32_10 and noise_uniform live in vv_common.h: the seeded token draws (vv_token_draw) share them
// grid ceil(total / 64) x 64 threads, total = B * kinds * quads; thread t = ((b * kinds) + kind) * quads + j
__global__ __launch_bounds__(64) void noise_normal_kernel(float* __restrict__ noise, int64_t ld_noise, float* __restrict__ sde_noise, int64_t ld_sde, int n,
                                                          int kinds, int quads, int total, const uint64_t* __restrict__ seeds, const int* __restrict__ frames) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= total) return;
  const int j = t % quads, bk = t / quads, kind = bk % kinds, b = bk / kinds;
  const uint64_t seed = seeds[b];
  const philox4 x = philox4x32_10(philox4{(unsigned)j, (unsigned)frames[b], (unsigned)kind, 0u}, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32));
  const float r0 = sqrtf(-2.0f * logf(noise_uniform(x.x))), a0 = 6.283185307179586f * noise_uniform(x.y);
  const float r1 = sqrtf(-2.0f * logf(noise_uniform(x.z))), a1 = 6.283185307179586f * noise_uniform(x.w);
  const float4 z = make_float4(r0 * cosf(a0), r0 * sinf(a0), r1 * cosf(a1), r1 * sinf(a1));
  float* row = kind == 0 ? noise + (int64_t)b * ld_noise : sde_noise + (int64_t)b * ld_sde + (int64_t)(kind - 1) * n;
  float* o = row + 4 * j;
  if (4 * j + 4 <= n && ((uintptr_t)o & 15) == 0) {
    *reinterpret_cast<float4*>(o) = z;
  } else {      // the row's last, partial quad, or a row that does not start on 16 bytes: elements >= n are dropped
    if (4 * j + 0 < n) o[0] = z.x;
    if (4 * j + 1 < n) o[1] = z.y;
    if (4 * j + 2 < n) o[2] = z.z;
    if (4 * j + 3 < n) o[3] = z.w;
  }
}

}  // namespace

extern "C" int vv_noise_normal(float* noise, int64_t ld_noise, float* sde_noise, int64_t ld_sde, int B, int n, int n_steps, const uint64_t* seeds,
                               const int* frames, vv_stream_t stream) {
  if (!noise || !seeds || !frames) return vv_set_error(VV_E_ARG, "vv_noise_normal: null noise, seeds or frames");
  if (B <= 0 || n <= 0 || n_steps < 0) return vv_set_error(VV_E_ARG, "vv_noise_normal: bad shape (B %d, n %d, n_steps %d)", B, n, n_steps);
  if (ld_noise < n) return vv_set_error(VV_E_ARG, "vv_noise_normal: ld_noise %lld < n %d", (long long)ld_noise, n);
  if (sde_noise && ld_sde < (int64_t)n_steps * n)
    return vv_set_error(VV_E_ARG, "vv_noise_normal: ld_sde %lld < n_steps * n = %lld", (long long)ld_sde, (long long)n_steps * n);
  const int kinds = 1 + (sde_noise ? n_steps : 0), quads = (n + 3) / 4;
  const int64_t total = (int64_t)B * kinds * quads;
  if (total > 0x7fffffff - 64) return vv_set_error(VV_E_ARG, "vv_noise_normal: %lld quads are more than one launch indexes", (long long)total);
  hipLaunchKernelGGL(noise_normal_kernel, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, (hipStream_t)stream, noise, ld_noise, sde_noise, ld_sde, n, kinds,
                     quads, (int)total, seeds, frames);
  VV_CHECK_LAUNCH("vv_noise_normal");
  return 0;
}

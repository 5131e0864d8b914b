// device-side helpers shared by the kernel units: bf16 weight words, packed-FMA K units, small vector loads / stores, the activations and the
// vv_linear epilogue (device code only).  A kernel unit reads these and does not restate them
#ifndef VV_DEVICE_H
#define VV_DEVICE_H
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "vv_hip.h"
#include "vv_common.h"

typedef unsigned short bf16_t;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 8 bf16 values of a 16-byte load as floats
__device__ __forceinline__ void unpack8(const u32x4 v, float (&o)[8]) {
  o[0] = __uint_as_float(v.x << 16); o[1] = __uint_as_float(v.x & 0xffff0000u);
  o[2] = __uint_as_float(v.y << 16); o[3] = __uint_as_float(v.y & 0xffff0000u);
  o[4] = __uint_as_float(v.z << 16); o[5] = __uint_as_float(v.z & 0xffff0000u);
  o[6] = __uint_as_float(v.w << 16); o[7] = __uint_as_float(v.w & 0xffff0000u);
}

// 16 bytes of weights.  NT: the matrix is streamed once per use and should not displace what stays in the caches; otherwise cacheable
template <bool NT>
__device__ __forceinline__ u32x4 ldw(const bf16_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}

// one lane's 8 weights of one K unit against an activation row: even / odd k accumulate separately (v_pk_fma_f32), j ascending
__device__ __forceinline__ void fma_unit(const u32x4 wv, const float (&x)[8], vf2& p) {
  float w[8];
  unpack8(wv, w);
#pragma unroll
  for (int j = 0; j < 8; j += 2) p = __builtin_elementwise_fma(vf2{w[j], w[j + 1]}, vf2{x[j], x[j + 1]}, p);
}

// v * gate + res as the generic epilogue (vv_epi_value below) rounds it: a product and a sum, never one FMA.  For the kernels whose epilogue is a
// compile-time cut of the sequence
__device__ __forceinline__ float gate_res(float v, float g, float r) {
#pragma clang fp contract(off)
  const float t = v * g;
  return t + r;
}

// two floats rounded to bf16 (nearest even), a in the low half
__device__ __forceinline__ unsigned int pack2(float a, float b) {
  const __hip_bfloat16 x = __float2bfloat16(a), y = __float2bfloat16(b);
  return (unsigned int)(*reinterpret_cast<const bf16_t*>(&x)) | ((unsigned int)(*reinterpret_cast<const bf16_t*>(&y)) << 16);
}
// the same rounding in integer arithmetic, for finite values only (a NaN's payload could carry into the exponent): bf16 bits of one float, and of
// two with a in the low half.  Kept apart from pack2: __float2bfloat16 handles NaN and compiles to other instructions
__device__ __forceinline__ unsigned bf16_bits(float f) {
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ unsigned bf16_bits2(float a, float b) { return bf16_bits(a) | (bf16_bits(b) << 16); }

// 8 e2m1 codes (one dword of a lane's MXFP4 load) under scale byte e -> the bf16 B fragment of one 32-wide k step
__device__ __forceinline__ bf16x8 mx_frag(unsigned codes, unsigned e) {
  const float s = __uint_as_float(e << 23);
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, s, 3);
  return bf16x8{p0[0], p0[1], p1[0], p1[1], p2[0], p2[1], p3[0], p3[1]};
}
__device__ __forceinline__ void ld4(const float* p, float (&o)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

// makes a loaded float4 / u32x4 opaque where it stands.  Behind a sched_barrier that follows the weight requests: hipcc otherwise hoists pieces
// of the arithmetic on v (and the waits they need) in front of the weight issue
#define VV_FENCE4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))

// the workgroup's place in a grid of nwg, renumbered so that the workgroups one XCD receives (ids = x mod 8) own consecutive tiles: the row
// tiles of one weight panel meet in one L2.  Bijective for every nwg: the first nwg % 8 XCDs hold one workgroup more than the others
__device__ __forceinline__ int xcd_remap(int orig, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

__device__ __forceinline__ float vv_silu(float v) { return v / (1.0f + expf(-v)); }
__device__ __forceinline__ float vv_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }     // exact (erf) form

// ---- what vv_linear computes after the dot product (include/vv_hip.h): + bias, GELU or SiLU(v) * v2, * gate, + res.  Every kernel that serves
// the run-time contract one output at a time reads the sequence from vv_epi_value; what is its own (an fp8 row scale or an rstd in front, the
// store behind) stays at the site.  The hot kernels' specialised epilogues are compile-time cuts of it and take its rounding from gate_res.

// The operands of one output (m, n), loaded where the sequence uses them
struct EpiAtUse {
  const vv_lin_args& a; int m, n;
  __device__ __forceinline__ float bias() const { return a.bias[n]; }
  __device__ __forceinline__ float gate() const { return a.gate_ld ? a.gate[(int64_t)m * a.gate_ld + n] : a.gate[n]; }
  __device__ __forceinline__ float res() const { return a.res[(int64_t)m * a.ldres + n]; }
};

// ... or fetched ahead of the dot product.  Their addresses are known before it is, and loads return in order: an operand load issued at epilogue
// time would sit behind the prefetched weights of the next row groups.  ROWSC: the kernel can meet fp8 row scales and fetches them alongside
struct EpiHeld {
  float b, g, r;               // bias, gate, residual: raw loads, an absent operand's value is never looked at
  __device__ __forceinline__ float bias() const { return b; }
  __device__ __forceinline__ float gate() const { return g; }
  __device__ __forceinline__ float res() const { return r; }
};
template <bool ROWSC> struct EpiOp : EpiHeld { float s, s2; };    // ... and the fp8 row scales of w and w2
template <> struct EpiOp<false> : EpiHeld {};
template <bool ROWSC>
__device__ __forceinline__ EpiOp<ROWSC> epi_load(const vv_lin_args& a, int m, int n) {
  // straight-line and use-free: an absent operand reads x[0] (always a valid address).  With a select per operand here the compiler waited for
  // each dword right away - draining every load issued before it - and a uniform branch per operand cut the issue sequence into blocks it
  // then reordered.
  EpiOp<ROWSC> e;
  const bool f8s = ROWSC && a.wdt == VV_FP8, f8d = f8s && a.w2;
  const float* pb = a.bias ? a.bias + n : a.x;
  const float* pg = a.gate ? a.gate + (a.gate_ld ? (int64_t)m * a.gate_ld + n : (int64_t)n) : a.x;
  const float* pr = a.res ? a.res + (int64_t)m * a.ldres + n : a.x;
  const float* ps = f8s ? a.wscale + n : a.x;
  const float* ps2 = f8d ? a.w2scale + n : a.x;
  e.b = *pb; e.g = *pg; e.r = *pr;
  if constexpr (ROWSC) { e.s = *ps; e.s2 = *ps2; }
  return e;
}

// one output: v the dot product, v2 the second matrix's (SwiGLU), o one of the operand sources above
template <class OPS>
__device__ __forceinline__ float vv_epi_value(const vv_lin_args& a, float v, float v2, const OPS& o) {
  if (a.bias) v += o.bias();
  if (a.act == VV_ACT_GELU) v = vv_gelu(v);
  else if (a.act == VV_ACT_SWIGLU) v = vv_silu(v) * v2;
  {
#pragma clang fp contract(off)      // a product and a sum, never one FMA: the rounding gate_res hands to the hot kernels
    if (a.gate) v *= o.gate();
    if (a.res) v += o.res();
  }
  return v;
}

#endif

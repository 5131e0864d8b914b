// device-side helpers shared by the kernel units: bf16 weight words, packed-FMA K units, small vector loads / stores (device code only)
#ifndef VV_DEVICE_H
#define VV_DEVICE_H
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

typedef unsigned short bf16_t;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float vf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

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

// v * gate + res as the generic epilogue rounds it: a product and a sum, never one FMA
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
__device__ __forceinline__ void ld4(const float* p, float (&o)[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
__device__ __forceinline__ void st4(float* p, const float (&o)[4]) { *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]); }

// makes a loaded float4 / u32x4 opaque where it stands.  Behind a sched_barrier that follows the weight requests: hipcc otherwise hoists pieces
// of the arithmetic on v (and the waits they need) in front of the weight issue
#define VV_FENCE4(v) asm volatile("" : "+v"((v).x), "+v"((v).y), "+v"((v).z), "+v"((v).w))

#endif

// vv_nf4_import.hip — a pre-quantized bitsandbytes 4-bit NF4 matrix (the checkpoint's packed bytes and block scales) into the engine's
// bf16 matrix and, where the layout holds the file's numbers exactly, its VV_NF4 companion (include/vv_hip.h).  Runs once per matrix at
// load time: memory-bound, one lane per 8 consecutive k of one row (4 packed bytes in, 16 bytes of bf16 and one dword of codes out).
// The codes are copied, never re-derived, and the scales are bnb's own fp32 absmax (decoded from the double-quantised form where the
// file has it): re-quantising the dequantised weights would give bf16(absmax), not absmax.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "vv_hip.h"
#include "vv_common.h"

namespace {

// bnb's block scale b: fp32 as stored, or (nested_map[code] * nested_absmax[b / nested_blocksize]) + nested_offset, each op rounded apart
__device__ __forceinline__ float block_absmax(const vv_nf4_src& s, int64_t b) {
#pragma clang fp contract(off)
  if (!s.nested_absmax) return static_cast<const float*>(s.absmax)[b];
  const float v = s.nested_map[static_cast<const uint8_t*>(s.absmax)[b]] * s.nested_absmax[b / s.nested_blocksize];
  return v + s.nested_offset;
}

__device__ __forceinline__ unsigned short nf4_value(const float* qmap, unsigned code, float absmax) {
#pragma clang fp contract(off)
  const __hip_bfloat16 b = __float2bfloat16(qmap[code] * absmax);     // round to nearest even
  return *reinterpret_cast<const unsigned short*>(&b);
}

// unit t = (row r, k0 = 8 * (t % units_per_row)); a row's last unit is short when k % 8 != 0.  vec: k % 8 == 0 and 4-byte aligned packed
// bytes (a unit is then one aligned dword); vec_w: ldw % 8 == 0 and 16-byte aligned w (a unit's bf16 values are one 16-byte store)
__global__ void __launch_bounds__(256) nf4_import_kernel(vv_nf4_src s, unsigned short* w, int64_t ldw, int row0, uint32_t* cq, float* cs,
                                                        int ku, int64_t units, int vec, int vec_w) {
  __shared__ float qmap[16];
  if (threadIdx.x < 16) qmap[threadIdx.x] = s.quant_map[threadIdx.x];
  __syncthreads();
  const int upr = (s.k + 7) / 8;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < units; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(t / upr), k0 = (int)(t % upr) * 8;
    const int cnt = min(8, s.k - k0);
    const int64_t j0 = (int64_t)r * s.k + k0;        // flat index of the unit's first element
    unsigned code[8];
    if (vec) {
      const uint32_t d = *reinterpret_cast<const uint32_t*>(s.packed + j0 / 2);
#pragma unroll
      for (int i = 0; i < 8; ++i) code[i] = (d >> (8 * (i / 2) + ((i & 1) ? 0 : 4))) & 15u;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t j = j0 + i;
        code[i] = i < cnt ? ((s.packed[j >> 1] >> ((j & 1) ? 0 : 4)) & 15u) : 0u;
      }
    }
    const int64_t b0 = j0 / s.blocksize, b1 = (j0 + cnt - 1) / s.blocksize;
    const float am0 = block_absmax(s, b0);
    unsigned short v[8];
    if (b0 == b1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = nf4_value(qmap, code[i], am0);
    } else {                                          // the unit straddles a block boundary (blocksize % 8 != 0 or k % 8 != 0)
      for (int i = 0; i < cnt; ++i) v[i] = nf4_value(qmap, code[i], block_absmax(s, (j0 + i) / s.blocksize));
    }
    unsigned short* dst = w + (int64_t)(row0 + r) * ldw + k0;
    if (vec_w && cnt == 8) {
      uint4 o;
      o.x = v[0] | ((uint32_t)v[1] << 16); o.y = v[2] | ((uint32_t)v[3] << 16);
      o.z = v[4] | ((uint32_t)v[5] << 16); o.w = v[6] | ((uint32_t)v[7] << 16);
      *reinterpret_cast<uint4*>(dst) = o;
    } else {
      for (int i = 0; i < cnt; ++i) dst[i] = v[i];
    }
    if (cq) {                                         // k % 64 == 0: every unit is whole and lies inside one 64-block of one bnb block
      const int row = row0 + r, q = row >> 2, rr = row & 3, u = k0 >> 9, l = (k0 & 511) >> 3;
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < 8; ++i) c |= code[i] << (4 * i);     // VV_NF4: nibble i of the dword is code k0 + i
      const int64_t unit = (int64_t)q * ku + u;
      cq[(unit * 64 + l) * 4 + rr] = c;
      if ((k0 & 63) == 0) cs[(unit * 4 + rr) * 8 + ((k0 & 511) >> 6)] = am0;
    }
  }
}

}  // namespace

extern "C" int vv_nf4_import(const vv_nf4_src* src, void* w, int64_t ldw, int row0, int rows_total, void* cq, float* cs, vv_stream_t stream) {
  if (!src || !w || !src->packed || !src->absmax || !src->quant_map || src->n <= 0 || src->k <= 0 || src->blocksize <= 0 || ldw < src->k ||
      row0 < 0 || rows_total < row0 || rows_total - row0 < src->n)
    return vv_set_error(VV_E_ARG, "vv_nf4_import: bad args (n %d k %d blocksize %d ldw %lld row0 %d rows_total %d)", src ? src->n : 0,
                        src ? src->k : 0, src ? src->blocksize : 0, (long long)ldw, row0, rows_total);
  if (src->nested_absmax && (!src->nested_map || src->nested_blocksize <= 0))
    return vv_set_error(VV_E_ARG, "vv_nf4_import: double quantisation needs nested_map and nested_blocksize > 0");
  if (!cq != !cs) return vv_set_error(VV_E_ARG, "vv_nf4_import: give both companion outputs (codes and scales) or neither");
  if (cq && (src->k % 64 || src->blocksize % 64 || src->k % src->blocksize))
    return vv_set_error(VV_E_ARG, "vv_nf4_import: the VV_NF4 companion needs k %% 64 == 0 and row-aligned blocks of a multiple of 64 (k %d, blocksize %d)",
                        src->k, src->blocksize);
  const int upr = (src->k + 7) / 8;
  const int64_t units = (int64_t)src->n * upr;
  const int vec = src->k % 8 == 0 && ((uintptr_t)src->packed % 4) == 0;
  const int vec_w = ldw % 8 == 0 && ((uintptr_t)w % 16) == 0;
  const int ku = (src->k + 511) / 512;
  int64_t blocks = (units + 255) / 256;
  if (blocks > 8192) blocks = 8192;                   // grid-stride the rest
  hipLaunchKernelGGL(nf4_import_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *src, (unsigned short*)w, ldw, row0,
                     (uint32_t*)cq, cs, ku, units, vec, vec_w);
  VV_CHECK_LAUNCH("vv_nf4_import");
  return 0;
}

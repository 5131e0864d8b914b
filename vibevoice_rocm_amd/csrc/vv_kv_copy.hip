// vv_kv_copy: slots [0, len) of one row of a KV cache into one row of another (vv_hip.h) - how a prefix store is filled from a cache and put
// back into one.  One launch over (32-key tile, KV head, layer), one tile per workgroup: the tile's k and v rows are contiguous on both
// sides and move as 16-byte words; the destination's transposed value tile is rebuilt from the v rows through LDS, so the source needs no
// vt and the v bytes are read from memory once.
#include "vv_common.h"

namespace {

typedef unsigned kvc_raw __attribute__((ext_vector_type(4)));

constexpr int KVC_ROW_W = 65;      // LDS row of one key: 64 dwords of bf16 pairs (head_dim 128) + 1 dword of padding

// grid (ceil(len / 32), kv_heads, layers), 256 threads.  row_bytes = head_dim x element size, a multiple of 16.
//   k, v:  the tile's nk <= 32 keys are nk * row_bytes contiguous bytes at the same tile offset in src and dst; thread i moves 16-byte word
//          i, i + 256, ... of each: every wave reads and writes 1 KB runs.
//   vt:    (bf16, head_dim 128 only) the tile is [128][32] bf16 = 512 16-byte words at the byte offset of the v tile; thread i writes word i
//          and i + 256, i.e. keys 8 q .. 8 q + 7 of row d = i / 4, q = i % 4, so a wave again writes one 1 KB run.  Its eight values come from
//          LDS rows 8 q + j, halfword d.  LDS banking of 32-bit accesses is (dword address) mod 32 within each 32-lane half: with 65 dwords
//          per key the half-wave's 32 reads touch 16 dwords on 16 different banks, 8 q + d / 2 + const (d and d + 1 share a dword: a
//          broadcast).  The v words go into LDS as 32-bit stores (key = i / 16, c = i % 16: dwords 65 key + 4 c + j); in any one store lanes c
//          and c + 8 of a half-wave would meet on a bank if they wrote the same j, so lanes with c >= 8 hold their four dwords rotated by
//          two (register j goes to dword (j + 2) % 4).  The compiler may pair the stores (ds_write2_b32): each half of a pair is banked
//          like a single store and the same argument holds.  Both statements are derived from the banking rule, not confirmed with the
//          SQ_LDS_BANK_CONFLICT counter; the kernel is a few microseconds per prompt either way.
//          A partial last tile writes columns < nk only: whole 16-byte words where 8 q + 8 <= nk, single bf16 below that.
__global__ __launch_bounds__(256) void kv_copy_kernel(vv_kv_args src, vv_kv_args dst, int src_row, int dst_row, int len, int row_bytes, int do_vt) {
  __shared__ unsigned sv[32 * KVC_ROW_W];
  const int tile = blockIdx.x, kvh = blockIdx.y, layer = blockIdx.z, tid = threadIdx.x;
  const int nk = min(32, len - tile * 32);
  const int64_t sb = ((((int64_t)layer * src.rows + src_row) * src.kv_heads + kvh) * src.s_max + (int64_t)tile * 32) * row_bytes;
  const int64_t db = ((((int64_t)layer * dst.rows + dst_row) * dst.kv_heads + kvh) * dst.s_max + (int64_t)tile * 32) * row_bytes;
  const kvc_raw* sk = reinterpret_cast<const kvc_raw*>(reinterpret_cast<const char*>(src.k) + sb);
  const kvc_raw* sv_g = reinterpret_cast<const kvc_raw*>(reinterpret_cast<const char*>(src.v) + sb);
  kvc_raw* dk = reinterpret_cast<kvc_raw*>(reinterpret_cast<char*>(dst.k) + db);
  kvc_raw* dv = reinterpret_cast<kvc_raw*>(reinterpret_cast<char*>(dst.v) + db);
  const int n16 = nk * (row_bytes >> 4);
  for (int i = tid; i < n16; i += 256) {
    const kvc_raw kw = sk[i], vw = sv_g[i];
    dk[i] = kw;
    dv[i] = vw;
    if (do_vt) {      // row_bytes == 256: 16 words per key
      const int key = i >> 4, c = i & 15, r = (c >> 3) << 1;
      unsigned* row = sv + key * KVC_ROW_W + 4 * c;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int jj = (j + r) & 3;
        row[jj] = jj == 0 ? vw.x : jj == 1 ? vw.y : jj == 2 ? vw.z : vw.w;
      }
    }
  }
  if (!do_vt) return;      // uniform over the grid
  __syncthreads();
  const unsigned short* sh = reinterpret_cast<const unsigned short*>(sv);
  char* vt = reinterpret_cast<char*>(dst.vt) + db;
  for (int i = tid; i < 512; i += 256) {
    const int d = i >> 2, k0 = (i & 3) * 8;
    if (k0 >= nk) continue;
    unsigned short e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = k0 + j < nk ? sh[(k0 + j) * (2 * KVC_ROW_W) + d] : (unsigned short)0;
    if (k0 + 8 <= nk) {
      *reinterpret_cast<kvc_raw*>(vt + (int64_t)i * 16) =
          kvc_raw{(unsigned)e[0] | ((unsigned)e[1] << 16), (unsigned)e[2] | ((unsigned)e[3] << 16), (unsigned)e[4] | ((unsigned)e[5] << 16), (unsigned)e[6] | ((unsigned)e[7] << 16)};
    } else {
      unsigned short* o = reinterpret_cast<unsigned short*>(vt + (int64_t)i * 16);
      for (int j = 0; j < nk - k0; ++j) o[j] = e[j];
    }
  }
}

}  // namespace

extern "C" int vv_kv_copy(const vv_kv* src, int src_row, const vv_kv* dst, int dst_row, int len, vv_stream_t stream) {
  if (!src || !dst) return vv_set_error(VV_E_ARG, "vv_kv_copy: null pointer");
  if (src->kvdt == VV_FP8 || dst->kvdt == VV_FP8)
    return vv_set_error(VV_E_UNSUPPORTED, "vv_kv_copy: an fp8 cache is filled through a bf16 staging cache and vv_kv_quantize");
  if ((src->kvdt != VV_F32 && src->kvdt != VV_BF16) || src->kvdt != dst->kvdt) return vv_set_error(VV_E_ARG, "vv_kv_copy: both caches must be fp32 or both bf16 (%d, %d)", src->kvdt, dst->kvdt);
  if (src->layers != dst->layers || src->kv_heads != dst->kv_heads || src->head_dim != dst->head_dim)
    return vv_set_error(VV_E_ARG, "vv_kv_copy: layers / kv_heads / head_dim differ (%d / %d / %d, %d / %d / %d)", src->layers, src->kv_heads, src->head_dim,
                        dst->layers, dst->kv_heads, dst->head_dim);
  if (src->layers <= 0 || src->kv_heads <= 0 || src->head_dim <= 0 || src->layers > 65535 || src->kv_heads > 65535) return vv_set_error(VV_E_ARG, "vv_kv_copy: bad cache shape");
  if (src_row < 0 || src_row >= src->rows || dst_row < 0 || dst_row >= dst->rows || len < 0 || len > src->s_max || len > dst->s_max)
    return vv_set_error(VV_E_ARG, "vv_kv_copy: row or len out of range (rows %d -> %d, len %d, s_max %d -> %d)", src_row, dst_row, len, src->s_max, dst->s_max);
  if (!src->k || !src->v || !dst->k || !dst->v) return vv_set_error(VV_E_ARG, "vv_kv_copy: null cache pointer");
  const int row_bytes = src->head_dim * (src->kvdt == VV_F32 ? 4 : 2);
  if (row_bytes % 16) return vv_set_error(VV_E_UNSUPPORTED, "vv_kv_copy: head_dim %d rows are no multiple of 16 bytes", src->head_dim);
  if (((uintptr_t)src->k % 16) || ((uintptr_t)src->v % 16) || ((uintptr_t)dst->k % 16) || ((uintptr_t)dst->v % 16) || ((uintptr_t)dst->vt % 16))
    return vv_set_error(VV_E_ARG, "vv_kv_copy: cache pointers must be 16-byte aligned");
  if (dst->vt && (dst->kvdt != VV_BF16 || dst->head_dim != 128 || dst->s_max % 32))
    return vv_set_error(VV_E_UNSUPPORTED, "vv_kv_copy: a destination with vt must be bf16 with head_dim 128 and s_max %% 32 == 0");
  if (len == 0) return 0;
  hipLaunchKernelGGL(kv_copy_kernel, dim3((len + 31) / 32, src->kv_heads, src->layers), dim3(256), 0, (hipStream_t)stream, vv_kv_args(*src), vv_kv_args(*dst), src_row,
                     dst_row, len, row_bytes, dst->vt ? 1 : 0);
  VV_CHECK_LAUNCH("vv_kv_copy");
  return 0;
}

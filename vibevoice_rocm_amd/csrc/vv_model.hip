// vv_model.hip — composite operators: each call enqueues the full launch sequence of one component of the
// per-frame loop (LLM step, diffusion-head sampling, acoustic decoder, semantic/acoustic encoder, connectors)
// on the caller's stream.  No host synchronisation, no allocation: capturable into one hipGraph per frame.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "vv_hip.h"
#include "vv_common.h"

namespace {

struct Carver {   // carve 256-byte aligned float buffers out of a caller-provided workspace
  char* p;
  explicit Carver(void* base) : p(reinterpret_cast<char*>(base)) {}
  float* take(size_t n_floats) {
    float* r = reinterpret_cast<float*>(p);
    p += (n_floats * sizeof(float) + 255) & ~(size_t)255;
    return r;
  }
};
inline size_t al(size_t n_floats) { return (n_floats * sizeof(float) + 255) & ~(size_t)255; }

inline vv_lin_args lin_base(const float* x, int64_t ldx, int m, const void* w, int n, int k, int wdt, float* out, int64_t ldo) {
  vv_lin_args a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.ldx = ldx; a.m = m; a.w = w; a.n = n; a.k = k; a.wdt = wdt; a.out = out; a.ldo = ldo;
  return a;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------
// Qwen2 decoder stack
// ---------------------------------------------------------------------------------------------------------------
// weight-only fp8, NF4, MXFP4 or MXFP6 companions (vv_w8; wq = VV_FP8 / VV_NF4 / VV_MXFP4 / VV_MXFP6, the descriptor's kind) replace the bf16 matrix on the weight-streaming
// GEMVs (<= 2 activation rows)
static inline void use_w8(vv_lin_args& a, int wq, const vv_w8& q, const vv_w8* q2 = nullptr) {
  if (a.m > 2 || !q.q || !q.scale || (a.w2 && (!q2 || !q2->q || !q2->scale))) return;
  a.w = q.q; a.wscale = q.scale; a.wdt = wq;
  if (a.w2) { a.w2 = q2->q; a.w2scale = q2->scale; }
}

// VV_WQ_NF4 / VV_WQ_MXFP4 / VV_WQ_MXFP6 (vv_hip.h) ride on a descriptor's wdt: every composite strips it once at entry into a local copy, so each wdt test below reads
// the matrix dtype, and keeps the companions' kind in `wq` (vv_wq_strip, vv_common.h); `fragq`: 0, or - VV_WQ_FRAG4 / VV_WQ_FRAG6 - the weight type the layers' f_* copies hold (VV_MXFP4_FRAG / VV_MXFP6_FRAG)
#define VV_WQ_STRIP(T, p)                                                   \
  T p##_plain_ = *(p);                                                      \
  const vv_wq_kind p##_kind_ = vv_wq_strip(&p##_plain_.wdt);                \
  const int wq = p##_kind_.wq;                                              \
  const int fragq = p##_kind_.fragq;                                        \
  p = &p##_plain_;                                                          \
  (void)wq; (void)fragq

// from this many rows on, a bf16-weight LLM forward is a prompt prefill: activations are cast to bf16 once per GEMM and both
// operands stream from global on the matrix cores with 128-row tiles (every weight fragment reused by 4 row tiles)
#define VV_PREFILL_ROWS 64
// decode attention over long contexts splits the keys over up to this many blocks per (row, q head) (vv_attn_decode.hip)
#define VV_ATT_ROWS 8
// ... and for the 9..16-row decode step (two row tiles of the matrix-core GEMV): the partials and tickets of a call are sized by its rows
static inline size_t att_rows(int R) { return (R > VV_ATT_ROWS && R <= 16) ? 16 : VV_ATT_ROWS; }
#define VV_ATT_MAX_SPLIT 16        // per-head kernel
#define VV_ATT_PART_SPLITS 128     // capacity of the partials workspace: the grouped kernel spreads long contexts over up to 128 splits per (row, KV head)

// split-K workspace of the row-batched decode step (vv_gemv_rows.hip): the widest non-dual matrix is the one that splits K
static size_t rows_part_floats(const vv_llm* m) {
  const int qkvd = (m->heads + 2 * m->kv_heads) * m->head_dim;
  const int n = qkvd > m->hidden ? qkvd : m->hidden;
  const size_t a = vv_gemv_rows_part_floats(n, 0), b = vv_gemv_rows_part_floats(m->inter, 1) / 8;     // the dual kernel splits K at most two ways
  return a > b ? a : b;
}
static size_t rows_tickets(const vv_llm* m) {
  const int qkvd = (m->heads + 2 * m->kv_heads) * m->head_dim;
  const int n = qkvd > m->inter ? qkvd : m->inter;
  return vv_gemv_rows_tickets(n > m->hidden ? n : m->hidden);
}

// A lean MXFP4 / MXFP6 LLM (vv_hip.h): the layers' bf16 pointers are NULL beside present MX companions.  1 = lean, 0 = every matrix resident, < 0 = a
// descriptor that is neither (VV_E_ARG) or a lean one whose shapes the GEMM on the codes does not take (VV_E_UNSUPPORTED).  Host only
static int llm_lean(const char* who, const vv_llm* m) {
  if (!m->layer || m->layers <= 0) return 0;
  int nul = 0;
  for (int l = 0; l < m->layers; ++l) {
    const vv_llm_layer& L = m->layer[l];
    nul += !L.wqkv + !L.wo + !L.wgate + !L.wup + !L.wdown;
  }
  if (!nul) return 0;
  if (nul != 5 * m->layers) return vv_set_error(VV_E_ARG, "%s: %d of %d LLM matrices are NULL: a lean mxfp4 / mxfp6 model has none of them, any other model all", who, nul, 5 * m->layers);
  const bool mx4 = (m->wdt & VV_WQ_MXFP4) != 0, mx6 = (m->wdt & VV_WQ_MXFP6) != 0;
  if (mx4 == mx6 || (m->wdt & 0xff) != VV_BF16) return vv_set_error(VV_E_ARG, "%s: NULL LLM matrices (the lean mode) need VV_BF16 | VV_WQ_MXFP4 or VV_BF16 | VV_WQ_MXFP6", who);
  const char* fmt = mx6 ? "mxfp6" : "mxfp4";
  for (int l = 0; l < m->layers; ++l) {
    const vv_llm_layer& L = m->layer[l];
    for (const vv_w8* q : {&L.q_qkv, &L.q_o, &L.q_gate, &L.q_up, &L.q_down})
      if (!q->q || !q->scale) return vv_set_error(VV_E_ARG, "%s: lean %s model: layer %d has neither a bf16 matrix nor an MX companion", who, fmt, l);
  }
  const int qd = m->heads * m->head_dim, qkvd = (m->heads + 2 * m->kv_heads) * m->head_dim;
  if (m->hidden % 128 || m->inter % 128 || qd % 128 || qkvd % 16)
    return vv_set_error(VV_E_UNSUPPORTED, "%s: lean %s model: hidden=%d inter=%d q width=%d must be multiples of 128 and the qkv width %d of 16 "
                        "(the GEMM on the codes takes n %% 16 == 0, k %% 128 == 0)", who, fmt, m->hidden, m->inter, qd, qkvd);
  return 1;
}

extern "C" size_t vv_llm_ws_bytes(const vv_llm* m, int R) {
  if (!m || R <= 0) return 0;
  const bool stage3 = R >= 3 && R < VV_PREFILL_ROWS && llm_lean("vv_llm_ws_bytes", m) == 1;      // a lean model casts to bf16 from 3 rows on
  const size_t qkv = (size_t)(m->heads + 2 * m->kv_heads) * m->head_dim;
  const size_t widest = (size_t)(m->inter > m->hidden ? m->inter : m->hidden);
  return al((size_t)R * m->hidden) + al((size_t)R * qkv) + al((size_t)R * m->heads * m->head_dim) + al((size_t)R * m->inter) +
         al((size_t)R * m->head_dim) + (R >= VV_PREFILL_ROWS || stage3 ? al((size_t)R * widest / 2 + 64) : 0) +
         al(att_rows(R) * m->heads * VV_ATT_PART_SPLITS * (m->head_dim + 2)) + al(att_rows(R) * m->heads) +                   // split-key decode attention
         ((R > 2 && R <= 16) ? al(rows_part_floats(m)) + al(rows_tickets(m)) : 0);                                           // split-K partials of the 3..8-row and the 9..16-row GEMV
}

// vv_llm_forward and vv_llm_prefill_packed: one layer loop.  lin_flags: ORed into the flags of the prefill branch's matrix-core linears
// (VV_LIN_PACKED or 0); sel (device int[nsel]) or null: the final norm runs on rows sel[i] alone, out is [nsel, hidden]
static int llm_forward(const char* who, const vv_llm* m, const vv_kv* kv, const float* x, int64_t ldx, int R, const int* lens,
                       const int* cache_rows, float* out, int64_t ldo, void* ws, vv_stream_t stream, int lin_flags, const int* sel, int nsel) {
  if (!m || !kv || !x || !lens || !ws || !m->layer) return vv_set_error(VV_E_ARG, "%s: null pointer", who);
  if (R <= 0) return vv_set_error(VV_E_ARG, "%s: R=%d", who, R);
  if (kv->layers != m->layers || kv->kv_heads != m->kv_heads || kv->head_dim != m->head_dim)
    return vv_set_error(VV_E_ARG, "%s: kv cache shape does not match the model", who);
  // cache_rows == NULL means row r owns cache row r (vv_hip.h): more rows than the cache has would be stored outside it
  if (!cache_rows && R > kv->rows) return vv_set_error(VV_E_ARG, "%s: cache_rows == NULL (row r owns cache row r) with R=%d > %d cache rows", who, R, kv->rows);
  const int lean_rc = llm_lean(who, m);
  if (lean_rc < 0) return lean_rc;
  const bool lean = lean_rc == 1;
  VV_WQ_STRIP(vv_llm, m);
  hipStream_t s = (hipStream_t)stream;
  const int H = m->hidden, d = m->head_dim, qd = m->heads * d, qkvd = (m->heads + 2 * m->kv_heads) * d;
  const bool decode = cache_rows == nullptr;      // R <= kv->rows: checked above
  if (lean && decode && R > 2 && R < VV_PREFILL_ROWS) {
    // lean: no bf16 matrix is resident, so a 3..8-row decode pass runs on the VV_MXFP4_FRAG / VV_MXFP6_FRAG copies or not at all, and 9..16 rows
    // not at all - said here, before the first launch
    const bool six = wq == VV_MXFP6;
    bool copies = fragq == (six ? VV_MXFP6_FRAG : VV_MXFP4_FRAG) && R <= 8;
    for (int l = 0; copies && l < m->layers; ++l) {
      const vv_llm_layer& L = m->layer[l];
      copies = L.f_qkv && L.f_o && L.f_gate && L.f_up && L.f_down;
    }
    if (!copies)
      return vv_set_error(VV_E_UNSUPPORTED, "%s: lean %s model (no bf16 LLM matrices): a decode pass of %d rows needs the %s copies of every layer "
                          "(%s=True) and 3..8 rows; 9..16 rows need bf16 copies, which the lean mode does not keep", who, six ? "mxfp6" : "mxfp4", R,
                          six ? "VV_MXFP6_FRAG" : "VV_MXFP4_FRAG", six ? "VV_WQ_FRAG6, mxfp6_row_batch" : "VV_WQ_FRAG4, mxfp4_row_batch");
  }
  Carver c(ws);
  float* h = c.take((size_t)R * H);
  float* qkv = c.take((size_t)R * qkvd);
  float* att = c.take((size_t)R * qd);
  float* act = c.take((size_t)R * m->inter);
  float* rope = c.take((size_t)R * d);
  // layer 0 reads the input embeddings where they lie (prologue and residual operand): no copy into the workspace
  const float* hin = x;
  int64_t ldh = ldx;
  VV_TRY(vv_rope_table(lens, m->inv_freq, R, d, rope, stream));
  // a lean model casts from 3 rows on in every non-decode pass: its matrices exist as codes alone, which the GEMMs of vv_gemm_mx.hip / vv_gemm_mx6.hip read
  const bool prefill = (R >= VV_PREFILL_ROWS || (lean && R > 2 && !decode)) && m->wdt == VV_BF16 && H % 16 == 0 && m->inter % 16 == 0 && qd % 16 == 0;
  void* xb = prefill ? (void*)c.take((size_t)R * (m->inter > H ? m->inter : H) / 2 + 64) : nullptr;
  float* att_part = c.take(att_rows(R) * m->heads * VV_ATT_PART_SPLITS * (d + 2));
  int* att_tickets = reinterpret_cast<int*>(c.take(att_rows(R) * m->heads));
  // contexts beyond ~1K keys: one block per (row, q head) would pull all of its K / V through a single CU (~95 GB/s: 8 us at S = 3000)
  // 9..16 rows: two row tiles of the same GEMV, when every layer has the bf16 fragment-major copies (no VV_WQ_FRAG4 / VV_WQ_FRAG6, whose copies are MX codes)
  bool rows16 = decode && R > 8 && R <= 16 && m->wdt == VV_BF16 && !fragq;
  for (int l = 0; rows16 && l < m->layers; ++l) {
    const vv_llm_layer& L = m->layer[l];
    rows16 = L.f_qkv && L.f_o && L.f_gate && L.f_up && L.f_down;
  }
  int att_split = 1;
  if (decode && (R <= VV_ATT_ROWS || rows16) && kv->s_max > 1024) {
    att_split = (kv->s_max + 511) / 512;
    if (att_split > VV_ATT_MAX_SPLIT) att_split = VV_ATT_MAX_SPLIT;
    hipError_t e = hipMemsetAsync(att_tickets, 0, att_rows(R) * m->heads * sizeof(int), s);
    if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  void* xb2 = prefill ? (void*)act : nullptr;      // bf16 SwiGLU output [R, inter] lives in the (otherwise unused) fp32 act buffer
  // 3..8 rows (dialogues batched into the row dimension): the matrix-core GEMV with its split-K workspace, fragment-major weights when the model has them
  const bool rows8 = (decode && R > 2 && R <= 8 && m->wdt == VV_BF16) || rows16;      // from here on "rows8" is either
  float* rpart = nullptr;
  int* rtick = nullptr;
  size_t rpart_n = 0, rtick_n = 0;
  if (rows8) {
    rpart_n = rows_part_floats(m); rtick_n = rows_tickets(m);
    rpart = c.take(rpart_n);
    rtick = reinterpret_cast<int*>(c.take(rtick_n));
    hipError_t e = hipMemsetAsync(rtick, 0, rtick_n * sizeof(int), s);
    if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
  }
  if (rows8) {      // the residual stream lives in h from the start: the split-K projections then accumulate into it in place (vv_gemv_rows.hip)
    VV_TRY(vv_copy_rows(x, ldx, h, H, R, H, stream));
    hin = h; ldh = H;
  }
  // rows8 with fp8 companions: f_* are the fragment-major copies of their codes (vv_llm_layer)
  auto lin = [&](vv_lin_args& a, const void* f1, const void* f2, const vv_w8* q1 = nullptr, const vv_w8* q2 = nullptr) -> int {
    if (!rows8) return vv_linear(&a, stream);
    // NF4 / MXFP4 companions never reach the 3..8-row kernel: f1 / f2 are then bf16 fragment-major copies of the effective matrices (or NULL) -
    // or, under VV_WQ_FRAG4 / VV_WQ_FRAG6, the VV_MXFP4_FRAG / VV_MXFP6_FRAG form of the MX companions
    return vv_linear_ws(&a, f1, f2, rpart, rpart_n, rtick, rtick_n, stream, wq == VV_FP8 ? q1 : nullptr, wq == VV_FP8 ? q2 : nullptr, fragq);
  };
  // lean, outside the rows kernel: the matrix is its MXFP4 / MXFP6 companion - under VV_LIN_W_MXGEMM / VV_LIN_W_MX6GEMM in the prefill branch, as the
  // streaming GEMV's operand at 1..2 rows (what use_w8 does for a model that has both)
  auto lean_w = [&](vv_lin_args& a, const vv_w8& q, const vv_w8* q2 = nullptr) {
    if (!lean || rows8) return;
    a.w = q.q; a.wscale = q.scale; a.wdt = wq;      // VV_MXFP4 or VV_MXFP6: llm_lean admits no other kind
    if (q2) { a.w2 = q2->q; a.w2scale = q2->scale; }
    if (prefill) a.flags |= wq == VV_MXFP6 ? VV_LIN_W_MX6GEMM : VV_LIN_W_MXGEMM;
  };
  for (int l = 0; l < m->layers; ++l) {
    const vv_llm_layer& L = m->layer[l];
    vv_lin_args a;
    if (prefill) {
      VV_TRY(vv_cast_rows_bf16(hin, ldh, R, H, VV_PRO_RMSNORM, L.ln1, m->rms_eps, xb, H, stream));
      a = lin_base((const float*)xb, H, R, L.wqkv, qkvd, H, m->wdt, qkv, qkvd);
      a.flags = VV_LIN_X_BF16 | lin_flags; a.bias = L.bqkv;
    } else {
      a = lin_base(hin, ldh, R, L.wqkv, qkvd, H, m->wdt, qkv, qkvd);
      a.pro = VV_PRO_RMSNORM; a.norm_w = L.ln1; a.eps = m->rms_eps; a.bias = L.bqkv;
      if (!rows8) use_w8(a, wq, L.q_qkv);
    }
    lean_w(a, L.q_qkv);
    VV_TRY(lin(a, L.f_qkv, nullptr, &L.q_qkv));
    if (decode) {
      VV_TRY(vv_attn_decode_ws(qkv, qkvd, R, m->heads, kv, l, rope, lens, att, qd, att_part, att_tickets, att_split, VV_ATT_PART_SPLITS, stream));   // decode: RoPE + append fused
    } else {
      VV_TRY(vv_rope_store(qkv, qkvd, R, m->heads, kv, l, rope, lens, cache_rows, stream));
      VV_TRY(vv_attn(qkv, qkvd, R, m->heads, kv, l, lens, cache_rows, att, qd, stream));
    }
    if (prefill) {
      VV_TRY(vv_cast_rows_bf16(att, qd, R, qd, VV_PRO_NONE, nullptr, 0.f, xb, qd, stream));
      a = lin_base((const float*)xb, qd, R, L.wo, H, qd, m->wdt, h, H);
      a.flags = VV_LIN_X_BF16 | lin_flags;
    } else {
      a = lin_base(att, qd, R, L.wo, H, qd, m->wdt, h, H);
      if (!rows8) use_w8(a, wq, L.q_o);
    }
    a.res = hin; a.ldres = ldh;
    lean_w(a, L.q_o);
    VV_TRY(lin(a, L.f_o, nullptr, &L.q_o));
    hin = h; ldh = H;
    if (prefill) {
      VV_TRY(vv_cast_rows_bf16(h, H, R, H, VV_PRO_RMSNORM, L.ln2, m->rms_eps, xb, H, stream));
      a = lin_base((const float*)xb, H, R, L.wgate, m->inter, H, m->wdt, act, m->inter);
      a.flags = VV_LIN_X_BF16 | lin_flags;
    } else {
      a = lin_base(h, H, R, L.wgate, m->inter, H, m->wdt, act, m->inter);
      a.pro = VV_PRO_RMSNORM; a.norm_w = L.ln2; a.eps = m->rms_eps;
    }
    a.w2 = L.wup; a.act = VV_ACT_SWIGLU;
    if (!prefill && !rows8) use_w8(a, wq, L.q_gate, &L.q_up);
    if (prefill) {            // the SwiGLU output is handed to the down projection in bf16: no separate cast pass
      a.out = reinterpret_cast<float*>(xb2); a.ldo = m->inter; a.flags |= VV_LIN_OUT_BF16;
    }
    lean_w(a, L.q_gate, &L.q_up);
    VV_TRY(lin(a, L.f_gate, L.f_up, &L.q_gate, &L.q_up));
    if (prefill) {
      a = lin_base((const float*)xb2, m->inter, R, L.wdown, H, m->inter, m->wdt, h, H);
      a.flags = VV_LIN_X_BF16 | lin_flags;
    } else {
      a = lin_base(act, m->inter, R, L.wdown, H, m->inter, m->wdt, h, H);
      if (!rows8) use_w8(a, wq, L.q_down);
    }
    a.res = h; a.ldres = H;
    lean_w(a, L.q_down);
    VV_TRY(lin(a, L.f_down, nullptr, &L.q_down));
  }
  if (!out) return 0;       // the caller runs the final norm itself (vv_llm_tail: norm + logits + token + bookkeeping in one launch)
  return vv_rmsnorm_rows(h, H, m->final_norm, m->rms_eps, sel ? nsel : R, H, out, ldo, s, sel);
}

extern "C" int vv_llm_forward(const vv_llm* m, const vv_kv* kv, const float* x, int64_t ldx, int R, const int* lens,
                              const int* cache_rows, float* out, int64_t ldo, void* ws, vv_stream_t stream) {
  return llm_forward("vv_llm_forward", m, kv, x, ldx, R, lens, cache_rows, out, ldo, ws, stream, 0, nullptr, 0);
}

extern "C" size_t vv_llm_prefill_packed_ws_bytes(const vv_llm* m, int R) { return vv_llm_ws_bytes(m, R); }

// Several prompts' rows in one pass: vv_llm_forward's prefill with VV_LIN_PACKED on its matrix-core linears and the final norm on the selected
// rows only.  Every row reads and writes its own (cache row, position) alone, so the rows of a pass may belong to any mix of cache rows
extern "C" int vv_llm_prefill_packed(const vv_llm* m, const vv_kv* kv, const float* x, int64_t ldx, int R, const int* lens, const int* cache_rows,
                                     const int* sel, int nsel, float* out, int64_t ldo, void* ws, vv_stream_t stream) {
  if (!cache_rows || !sel || !out) return vv_set_error(VV_E_ARG, "vv_llm_prefill_packed: null pointer");
  if (nsel <= 0) return vv_set_error(VV_E_ARG, "vv_llm_prefill_packed: nsel=%d", nsel);
  if (kv && kv->kvdt == VV_FP8) return vv_set_error(VV_E_UNSUPPORTED, "vv_llm_prefill_packed: an fp8 KV cache takes no prompt rows (prefill a bf16 cache, then vv_kv_quantize)");
  return llm_forward("vv_llm_prefill_packed", m, kv, x, ldx, R, lens, cache_rows, out, ldo, ws, stream, VV_LIN_PACKED, sel, nsel);
}

// ---------------------------------------------------------------------------------------------------------------
// diffusion head + DPM-Solver++ sampling
// ---------------------------------------------------------------------------------------------------------------
// ---- the samplers' workspace and stage choice: one copy each, for the launch path and for vv_head_ws_layout / vv_head_sample_route ----
// byte offsets of the regions a sampler carves out of its workspace; none = the form has no such region
struct HeadWs {
  static constexpr size_t none = ~(size_t)0;
  size_t c0, c, mod[16], modf, hb[2], act, Xs, Ms, NX, v, xb[2], mb[2], rpart, rtick, end;
  size_t rpart_n, rtick_n;       // floats / ints of the rows GEMV's split-K partials and tickets (batched form)
};
struct OffCarver {               // Carver on offsets
  size_t o = 0;
  size_t take(size_t n_floats) { const size_t r = o; o += al(n_floats); return r; }
};

// vv_head_sample (h with the companion flags stripped)
static HeadWs head_carve_single(const vv_head* h, int n_steps) {
  const size_t D = h->D, R = 2 * (size_t)n_steps > 8 ? 2 * (size_t)n_steps : 8;
  HeadWs o;
  OffCarver cv;
  o.c0 = cv.take(8 * D);
  o.c = cv.take(R * D);
  for (int l = 0; l < 16; ++l) o.mod[l] = l < h->layers ? cv.take(R * 3 * D) : HeadWs::none;
  o.modf = cv.take(R * 2 * D);
  o.hb[0] = cv.take(8 * D);
  o.act = cv.take(8 * (size_t)h->ffn);
  o.v = cv.take(8 * (size_t)h->latent);
  o.xb[0] = cv.take(h->latent); o.xb[1] = cv.take(h->latent);
  o.mb[0] = cv.take(h->latent); o.mb[1] = cv.take(h->latent);
  o.hb[1] = cv.take(8 * D);
  o.Xs = cv.take(D + (size_t)h->latent);
  o.Ms = cv.take(D + (size_t)h->latent);
  o.NX = o.rpart = o.rtick = HeadWs::none; o.rpart_n = o.rtick_n = 0;
  o.end = cv.o;
  return o;
}

// vv_head_sample_batch(_sde / _cfg): rows [2 B] where the single-utterance form has 2; NX (SDE) carved last, so the ODE layout is a prefix
static HeadWs head_carve_batch(const vv_head* h, int n_steps, int B, bool sde) {
  const size_t D = h->D, R = (size_t)2 * B * n_steps, sst = D + (size_t)h->latent;
  const size_t HR = B <= 4 ? 8 : (size_t)2 * B;          // hidden / act / c0 rows: 8 as ever up to 4 utterances, 2 B beyond
  HeadWs o;
  OffCarver cv;
  o.c0 = cv.take(HR * D);
  o.c = cv.take(R * D);
  for (int l = 0; l < 16; ++l) o.mod[l] = l < h->layers ? cv.take(R * 3 * D) : HeadWs::none;
  o.modf = cv.take(R * 2 * D);
  o.hb[0] = cv.take(HR * D); o.hb[1] = cv.take(HR * D);
  o.act = cv.take(HR * (size_t)h->ffn);
  o.Xs = cv.take((size_t)B * sst);
  o.Ms = cv.take((size_t)B * sst);
  o.rpart_n = vv_gemv_rows_part_floats(h->D, 0); o.rtick_n = vv_gemv_rows_tickets(h->ffn);
  o.rpart = cv.take(o.rpart_n);
  o.rtick = cv.take(o.rtick_n);
  o.NX = sde ? cv.take((size_t)B * n_steps * sst) : HeadWs::none;
  o.v = o.xb[0] = o.xb[1] = o.mb[0] = o.mb[1] = HeadWs::none;
  o.end = cv.o;
  return o;
}

extern "C" size_t vv_head_ws_bytes(const vv_head* h, int n_steps) {
  if (!h || n_steps <= 0) return 0;
  if (h->layers < 0 || h->layers > 16) return 0;
  VV_WQ_STRIP(vv_head, h);
  return head_carve_single(h, n_steps).end;
}

// shared body: rows R (<= 8), modulation tables mod[l] [*, 3D] / modf [*, 2D] with row offset `mrow`
static int head_body(const vv_head* h, int wq, const float* x, int64_t ldx, int R, float* const* mod, const float* modf, int64_t mrow,
                     float* hcur, float* act, float* v, vv_stream_t stream) {
  const int D = h->D;
  vv_lin_args a;
  if (x) {                                   // x == NULL: hcur = noisy_images_proj(x) was already produced (vv_dpm_proj)
    a = lin_base(x, ldx, R, h->noisy_proj, D, h->latent, h->wdt, hcur, D);
    VV_TRY(vv_linear(&a, stream));
  }
  for (int l = 0; l < h->layers; ++l) {
    const vv_head_layer& L = h->layer[l];
    const float* ml = mod[l] + mrow * 3 * D;
    a = lin_base(hcur, D, R, L.wgate, h->ffn, D, h->wdt, act, h->ffn);
    a.pro = VV_PRO_RMSNORM; a.norm_w = L.norm_w; a.eps = h->eps;
    a.mod_shift = ml; a.mod_scale = ml + D; a.ld_mod = 3 * D;
    a.w2 = L.wup; a.act = VV_ACT_SWIGLU;
    use_w8(a, wq, L.q_gate, &L.q_up);
    VV_TRY(vv_linear(&a, stream));
    a = lin_base(act, h->ffn, R, L.wdown, D, h->ffn, h->wdt, hcur, D);
    a.gate = ml + 2 * D; a.gate_ld = 3 * D; a.res = hcur; a.ldres = D;
    use_w8(a, wq, L.q_down);
    VV_TRY(vv_linear(&a, stream));
  }
  const float* mf = modf + mrow * 2 * D;
  a = lin_base(hcur, D, R, h->final_linear, h->latent, D, h->wdt, v, h->latent);
  a.pro = VV_PRO_RMSNORM; a.norm_w = nullptr; a.eps = h->eps;
  a.mod_shift = mf; a.mod_scale = mf + D; a.ld_mod = 2 * D;
  return vv_linear(&a, stream);
}

// c: fp32 rows (presilu false: SiLU applied as the GEMM prologue) or, with c_bf16, SiLU'd rows already rounded to bf16 (the operand the
// matrix-core path would round to anyway; the >= 32-tile adaLN GEMMs then run on the LDS-tiled kernel)
static int head_modulations(const vv_head* h, const float* c, int rows, float* const* mod, float* modf, bool presilu, bool c_bf16, vv_stream_t stream) {
  const int D = h->D;
  if (presilu && c_bf16) {     // the per-frame form (rows = 2 * n_steps bf16 conditioning rows): every matrix in one launch (vv_fused.hip)
    const int one = vv_head_modulations_fused(h, c, rows, mod, modf, (hipStream_t)stream);
    if (one) return one < 0 ? one : 0;
  }
  for (int l = 0; l < h->layers; ++l) {
    vv_lin_args a = lin_base(c, D, rows, h->layer[l].adaln, 3 * D, D, h->wdt, mod[l], 3 * D);
    a.pro = presilu ? VV_PRO_NONE : VV_PRO_SILU;
    if (c_bf16) a.flags = VV_LIN_X_BF16;
    VV_TRY(vv_linear(&a, stream));
  }
  vv_lin_args a = lin_base(c, D, rows, h->final_adaln, 2 * D, D, h->wdt, modf, 2 * D);
  a.pro = presilu ? VV_PRO_NONE : VV_PRO_SILU;
  if (c_bf16) a.flags = VV_LIN_X_BF16;
  return vv_linear(&a, stream);
}

extern "C" int vv_head_forward(const vv_head* h, const float* x, const float* temb_rows, const float* cond, int R, float* v,
                               void* ws, vv_stream_t stream) {
  if (!h || !x || !temb_rows || !cond || !v || !ws) return vv_set_error(VV_E_ARG, "vv_head_forward: null pointer");
  if (R <= 0 || R > 8 || h->layers > 16) return vv_set_error(VV_E_ARG, "vv_head_forward: R=%d (1..8)", R);
  VV_WQ_STRIP(vv_head, h);
  const int D = h->D;
  Carver cv(ws);
  float* c0 = cv.take(8 * (size_t)D);
  float* c = cv.take(8 * (size_t)D);
  float* mod[16];
  for (int l = 0; l < h->layers; ++l) mod[l] = cv.take(8 * 3 * (size_t)D);
  float* modf = cv.take(8 * 2 * (size_t)D);
  float* hcur = cv.take(8 * (size_t)D);
  float* act = cv.take(8 * (size_t)h->ffn);
  vv_lin_args a = lin_base(cond, h->cond_dim, R, h->cond_proj, D, h->cond_dim, h->wdt, c0, D);
  VV_TRY(vv_linear(&a, stream));
  // c[r] = c0[r] + temb_rows[r]: rows_b = R with a single "step" whose b-row is row r -> use add_rows twice-free form
  for (int r = 0; r < R; ++r) VV_TRY(vv_add_rows(c0 + (size_t)r * D, D, temb_rows + (size_t)r * D, D, c + (size_t)r * D, 1, 1, D, stream));
  VV_TRY(head_modulations(h, c, R, mod, modf, false, false, stream));
  return head_body(h, wq, x, h->latent, R, mod, modf, 0, hcur, act, v, stream);
}

// ---- the samplers' stage choice: one copy, for the launch path and for vv_head_sample_route ----
// the stage kernels a sampler call takes
struct HeadRoute {
  int B;           // 0: vv_head_sample
  int pre_ku;      // head_pre_kernel<KU>, 0: vv_linear + vv_add_rows_silu(_bf16) (+ head_init_kernel where the fused boundary follows)
  bool cb;         // conditioning rows c in bf16
  int mod_nst;     // 12: adaln_lds_kernel<12>, 28: adaln_all_kernel<28, 1>, 0: one vv_linear per adaLN matrix
  int step_ku;     // head_boundary(_cfg)_kernel<KU, SDE>, 0: the three-launch form (vv_dpm_proj + the FinalLayer vv_linear)
  bool sde_proj;   // head_sde_proj_kernel in front of the loop (batched form with variance noise)
  bool sde;        // steps with coef[i].cn != 0 run the SDE instantiation of the boundary
  bool cfg;        // head_boundary_cfg_kernel
  bool f32;        // fp32 weights (head_init_kernel<float>)
};

// vv_head_sample's refusals and choices (noise and latent_out are the caller's to check).  0, or the call's error
static int head_single_decide(const vv_head* h, const float* cond2, int64_t ld_cond, const float* temb, const vv_dpm_coef* coef, int n_steps,
                              bool sde_given, const void* ws, HeadRoute* r) {
  if (!h || !cond2 || !temb || !coef || !ws) return vv_set_error(VV_E_ARG, "vv_head_sample: null pointer");
  if (n_steps <= 0 || h->layers > 16) return vv_set_error(VV_E_ARG, "vv_head_sample: bad n_steps/layers");
  VV_WQ_STRIP(vv_head, h);
  const char* c = reinterpret_cast<const char*>(ws) + head_carve_single(h, n_steps).c;
  r->B = 0; r->f32 = h->wdt == VV_F32; r->sde_proj = r->sde = r->cfg = false;
  r->cb = h->wdt == VV_BF16 && 2 * n_steps > 8 && h->D % 32 == 0 && ((uintptr_t)c % 16 == 0);
  bool ode = !sde_given;
  for (int i = 0; i < n_steps && ode; ++i) ode = coef[i].cn == 0.f;
  r->step_ku = (ode && vv_head_boundary_supported(h)) ? vv_head_boundary_decide(h) : 0;
  r->pre_ku = (r->cb && r->step_ku) ? vv_head_pre_decide(h, cond2, ld_cond, temb, n_steps, c) : 0;
  r->mod_nst = r->cb ? vv_head_modulations_decide(h, c, 2 * n_steps) : 0;
  return 0;
}

// the batched samplers' (fn; sde_fn false: vv_head_sample_batch, which refuses SDE coefficients)
static int head_batch_decide(const char* fn, bool sde_fn, const vv_head* h, const float* cond, const float* temb, const vv_dpm_coef* coef, int n_steps,
                             int B, bool sde_given, int64_t ld_sde, bool cfg, const void* ws, HeadRoute* r) {
  if (!h || !cond || !temb || !coef || !ws) return vv_set_error(VV_E_ARG, "%s: null pointer", fn);
  if (n_steps <= 0 || h->layers > 16 || B <= 0 || B > 8) return vv_set_error(VV_E_ARG, "%s: n_steps=%d layers=%d B=%d (1..8)", fn, n_steps, h->layers, B);
  VV_WQ_STRIP(vv_head, h);
  bool ode = true;
  for (int i = 0; i < n_steps && ode; ++i) ode = coef[i].cn == 0.f;
  if (!sde_fn && !ode) return vv_set_error(VV_E_UNSUPPORTED, "vv_head_sample_batch: the SDE solver is served by vv_head_sample_batch_sde");
  if (sde_given && ld_sde < (int64_t)n_steps * h->latent) return vv_set_error(VV_E_ARG, "%s: ld_sde=%lld < n_steps * latent", fn, (long long)ld_sde);
  if (!sde_given && !ode) return vv_set_error(VV_E_ARG, "%s: the SDE solver step needs its variance noise", fn);
  if (h->wdt != VV_BF16 || !vv_head_boundary_supported(h) || h->D % 32 || !vv_head_boundary_decide(h))
    return vv_set_error(VV_E_UNSUPPORTED, "%s: needs bf16 weights and the fused solver boundary (vv_head.fused_g)", fn);
  const char* c = reinterpret_cast<const char*>(ws) + head_carve_batch(h, n_steps, B, sde_given).c;
  r->B = B; r->f32 = false; r->cb = true; r->pre_ku = 0; r->cfg = cfg;
  r->mod_nst = vv_head_modulations_decide(h, c, 2 * B * n_steps);
  r->step_ku = vv_head_boundary_decide(h);
  r->sde_proj = sde_given; r->sde = sde_given && !ode;
  return 0;
}

extern "C" int vv_head_sample_route(const vv_head* h, const float* cond, int64_t ld_cond, const float* temb, const vv_dpm_coef* coef, int n_steps, int B,
                                    int sde, const float* cfg_rows, const void* ws, char* name, int cap) {
  if (!name || cap <= 0) return vv_set_error(VV_E_ARG, "vv_head_sample_route: no room for the name");
  name[0] = 0;
  HeadRoute r;
  if (B < 0) return vv_set_error(VV_E_ARG, "vv_head_sample_route: B=%d", B);
  if (B == 0) {
    if (cfg_rows) return vv_set_error(VV_E_ARG, "vv_head_sample_route: vv_head_sample takes no cfg_rows");
    VV_TRY(head_single_decide(h, cond, ld_cond, temb, coef, n_steps, sde != 0, ws, &r));
  } else {
    const char* fn = cfg_rows ? "vv_head_sample_batch_cfg" : sde ? "vv_head_sample_batch_sde" : "vv_head_sample_batch";
    VV_TRY(head_batch_decide(fn, cfg_rows || sde, h, cond, temb, coef, n_steps, B, sde != 0, INT64_MAX, cfg_rows != nullptr, ws, &r));
  }
  const char* wt = r.f32 ? "f32" : "bf16";
  char pre[96], mod[40], step[48];
  if (r.pre_ku) snprintf(pre, sizeof pre, "head_pre<ku=%d>", r.pre_ku);
  else
    snprintf(pre, sizeof pre, "linear+add_rows_silu%s%s%s%s%s%s%s", r.cb ? "_bf16" : "", r.step_ku ? "+head_init<" : "", r.step_ku ? wt : "", r.step_ku ? ">" : "",
             r.sde_proj ? "+head_sde_proj<" : "", r.sde_proj ? wt : "", r.sde_proj ? ">" : "");
  if (r.mod_nst == 12) snprintf(mod, sizeof mod, "adaln_lds<nst=12>");
  else if (r.mod_nst == 28) snprintf(mod, sizeof mod, "adaln_all<nst=28,nm=1>");
  else snprintf(mod, sizeof mod, "linear");
  if (r.step_ku) snprintf(step, sizeof step, "boundary<ku=%d,sde=%d,cfg=%d>", r.step_ku, (int)r.sde, (int)r.cfg);
  else snprintf(step, sizeof step, "dpm_proj");
  snprintf(name, (size_t)cap, "pre=%s mod=%s step=%s", pre, mod, step);
  return 0;
}

extern "C" int vv_head_ws_layout(const vv_head* h, int n_steps, int B, int sde, int64_t* off, int cap) {
  if (!h || !off) return vv_set_error(VV_E_ARG, "vv_head_ws_layout: null pointer");
  if (n_steps <= 0 || h->layers < 0 || h->layers > 16 || B < 0 || B > 8) return vv_set_error(VV_E_ARG, "vv_head_ws_layout: n_steps=%d layers=%d B=%d (0..8)", n_steps, h->layers, B);
  if (B == 0 && sde) return vv_set_error(VV_E_ARG, "vv_head_ws_layout: vv_head_sample keeps no variance noise in its workspace (sde with B = 0)");
  const int n = h->layers + 10 + (B == 0 ? 5 : 0);
  if (cap < n) return vv_set_error(VV_E_ARG, "vv_head_ws_layout: room for %d offsets, the layout has %d", cap, n);
  VV_WQ_STRIP(vv_head, h);
  const HeadWs o = B == 0 ? head_carve_single(h, n_steps) : head_carve_batch(h, n_steps, B, sde != 0);
  auto put = [](size_t v) { return v == HeadWs::none ? (int64_t)-1 : (int64_t)v; };
  int k = 0;
  off[k++] = put(o.c0); off[k++] = put(o.c);
  for (int l = 0; l < h->layers; ++l) off[k++] = put(o.mod[l]);
  off[k++] = put(o.modf); off[k++] = put(o.hb[0]); off[k++] = put(o.hb[1]); off[k++] = put(o.act);
  off[k++] = put(o.Xs); off[k++] = put(o.Ms); off[k++] = put(o.NX);
  if (B == 0) { off[k++] = put(o.v); off[k++] = put(o.xb[0]); off[k++] = put(o.xb[1]); off[k++] = put(o.mb[0]); off[k++] = put(o.mb[1]); }
  off[k++] = put(o.end);
  return k;
}

extern "C" int vv_head_sample(const vv_head* h, const float* cond2, int64_t ld_cond, const float* noise, const float* temb,
                              const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, void* ws,
                              const float* sde_noise, vv_stream_t stream) {
  if (!noise || !latent_out) return vv_set_error(VV_E_ARG, "vv_head_sample: null pointer");
  HeadRoute rt;
  VV_TRY(head_single_decide(h, cond2, ld_cond, temb, coef, n_steps, sde_noise != nullptr, ws, &rt));
  VV_WQ_STRIP(vv_head, h);
  hipStream_t s = (hipStream_t)stream;
  const int D = h->D;
  const HeadWs o = head_carve_single(h, n_steps);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + off); };
  float* c0 = at(o.c0);
  float* c = at(o.c);
  float* mod[16];
  for (int l = 0; l < h->layers; ++l) mod[l] = at(o.mod[l]);
  float* modf = at(o.modf);
  float* hcur = at(o.hb[0]);
  float* act = at(o.act);
  float* v = at(o.v);
  float* xb[2] = {at(o.xb[0]), at(o.xb[1])};       // x and x0-history are double-buffered per step
  float* mb[2] = {at(o.mb[0]), at(o.mb[1])};
  float* hcur2 = at(o.hb[1]);
  float* Xs = at(o.Xs);
  float* Ms = at(o.Ms);
  // step-invariant work hoisted out of the loop: cond_proj, silu(cond_proj(cond) + t_emb(t_i)), all adaLN modulations
  const bool cb = rt.cb;
  // the ODE solver on the fused boundary: cond_proj, the row expansion and the solver-state initialisation are one launch (vv_fused.hip)
  int pre = 0;
  if (rt.pre_ku) {
    pre = vv_head_pre_fused(h, cond2, ld_cond, temb, n_steps, c, noise, Xs, Ms, hcur, D, s);
    if (pre < 0) return pre;
  }
  vv_lin_args a;
  if (!pre) {
    a = lin_base(cond2, ld_cond, 2, h->cond_proj, D, h->cond_dim, h->wdt, c0, D);
    VV_TRY(vv_linear(&a, stream));
    if (cb) VV_TRY(vv_add_rows_silu_bf16(c0, D, temb, D, c, 2 * n_steps, 2, D, stream));
    else VV_TRY(vv_add_rows_silu(c0, D, temb, D, c, 2 * n_steps, 2, D, stream));
  }
  VV_TRY(head_modulations(h, c, 2 * n_steps, mod, modf, true, cb, stream));
  if (rt.step_ku) {          // the SDE solver (variance noise per step) keeps the three-launch boundary
    // one launch per step boundary: FinalLayer + CFG + DPM-Solver++ update + next noisy_images_proj as ONE GEMV over G = [P F ; F]
    // with the solver in its epilogue (vv_fused.hip).  The hidden rows alternate between two buffers: the boundary kernel of step i
    // reads the rows the layers of step i worked on while it writes the rows step i + 1 starts from.
    float* hb[2] = {hcur, hcur2};
    if (!pre) VV_TRY(vv_head_init_fused(h, noise, Xs, Ms, hb[0], D, s));
    for (int i = 0; i < n_steps; ++i) {
      float* hc = hb[i & 1];
      for (int l = 0; l < h->layers; ++l) {
        const vv_head_layer& L = h->layer[l];
        const float* ml = mod[l] + (size_t)2 * i * 3 * D;
        a = lin_base(hc, D, 2, L.wgate, h->ffn, D, h->wdt, act, h->ffn);
        a.pro = VV_PRO_RMSNORM; a.norm_w = L.norm_w; a.eps = h->eps;
        a.mod_shift = ml; a.mod_scale = ml + D; a.ld_mod = 3 * D;
        a.w2 = L.wup; a.act = VV_ACT_SWIGLU; a.flags = VV_LIN_W_REUSED;
        use_w8(a, wq, L.q_gate, &L.q_up);
        VV_TRY(vv_linear(&a, stream));
        a = lin_base(act, h->ffn, 2, L.wdown, D, h->ffn, h->wdt, hc, D);
        a.gate = ml + 2 * D; a.gate_ld = 3 * D; a.res = hc; a.ldres = D; a.flags = VV_LIN_W_REUSED;
        use_w8(a, wq, L.q_down);
        VV_TRY(vv_linear(&a, stream));
      }
      const float* mf = modf + (size_t)2 * i * 2 * D;
      VV_TRY(vv_head_boundary_fused(h, hc, D, mf, mf + D, 2 * D, cfg_scale, &coef[i], Xs, Ms, hb[(i + 1) & 1], D, latent_out, s));
    }
    return 0;
  }
  for (int i = 0; i <= n_steps; ++i) {
    // step boundary: solver update of the previous step's v (none before step 0) fused with this step's noisy_images_proj
    const float* xin = (i == 0) ? noise : xb[(i - 1) & 1];
    float* xout = (i == n_steps) ? latent_out : xb[i & 1];
    VV_TRY(vv_dpm_proj(i == 0 ? nullptr : v, h->latent, cfg_scale, i == 0 ? nullptr : &coef[i - 1], xin, mb[(i - 1) & 1], xout, mb[i & 1],
                       i == n_steps ? nullptr : h->noisy_proj, h->wdt, h->latent, D, hcur, D, 2,
                       (sde_noise && i > 0) ? sde_noise + (size_t)(i - 1) * h->latent : nullptr, stream));
    if (i == n_steps) break;
    VV_TRY(head_body(h, wq, nullptr, 0, 2, mod, modf, 2 * (int64_t)i, hcur, act, v, stream));
  }
  (void)s;
  return 0;
}

// B utterances per call: rows [2 B] everywhere the single-utterance sampler has 2; conditioning rows laid out [step][2 B]
extern "C" size_t vv_head_ws_bytes_batch(const vv_head* h, int n_steps, int B) {
  if (!h || n_steps <= 0 || B <= 0 || B > 8) return 0;
  if (h->layers < 0 || h->layers > 16) return 0;
  VV_WQ_STRIP(vv_head, h);
  return head_carve_batch(h, n_steps, B, false).end;
}

// the SDE form: the same workspace with the variance noise of every step of every utterance in state space, NX [B][n_steps][D + latent], at its end
extern "C" size_t vv_head_ws_bytes_batch_sde(const vv_head* h, int n_steps, int B) {
  if (!vv_head_ws_bytes_batch(h, n_steps, B)) return 0;       // its refusals
  VV_WQ_STRIP(vv_head, h);
  return head_carve_batch(h, n_steps, B, true).end;
}

// sde_noise == NULL: the ODE solver (every launch identical to vv_head_sample_batch's); else [B][n_steps][latent] at utterance stride ld_sde,
// step i of utterance b adding coef[i].cn * sde_noise[b][i] to x (the noise vv_head_sample takes after step i).  sde_fn == NULL: the ODE-only
// entry point vv_head_sample_batch, which refuses SDE coefficients
static int head_sample_batch(const char* sde_fn, const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                             const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, int64_t ld_latent, int B, void* ws,
                             const float* sde_noise, int64_t ld_sde, vv_stream_t stream, const float* cfg_rows = nullptr) {
  const char* fn = sde_fn ? sde_fn : "vv_head_sample_batch";
  if (!noise || !latent_out) return vv_set_error(VV_E_ARG, "%s: null pointer", fn);
  HeadRoute rt;
  VV_TRY(head_batch_decide(fn, sde_fn != nullptr, h, cond, temb, coef, n_steps, B, sde_noise != nullptr, ld_sde, cfg_rows != nullptr, ws, &rt));
  VV_WQ_STRIP(vv_head, h);
  const bool f8q = wq == VV_FP8;                  // NF4 companions: the bf16 matrices (and their bf16 fragment-major copies) serve these rows
  hipStream_t s = (hipStream_t)stream;
  const int D = h->D, R2 = 2 * B;
  const size_t R = (size_t)R2 * n_steps;
  const HeadWs o = head_carve_batch(h, n_steps, B, sde_noise != nullptr);
  auto at = [&](size_t off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + off); };
  float* c0 = at(o.c0);
  float* c = at(o.c);
  float* mod[16];
  for (int l = 0; l < h->layers; ++l) mod[l] = at(o.mod[l]);
  float* modf = at(o.modf);
  float* hb[2] = {at(o.hb[0]), at(o.hb[1])};
  float* act = at(o.act);
  const int64_t sst = D + h->latent;
  float* Xs = at(o.Xs);
  float* Ms = at(o.Ms);
  const size_t rpart_n = o.rpart_n, rtick_n = o.rtick_n;
  float* rpart = at(o.rpart);
  int* rtick = reinterpret_cast<int*>(at(o.rtick));
  if (hipMemsetAsync(rtick, 0, rtick_n * sizeof(int), s) != hipSuccess) return vv_set_error(VV_E_HIP, "%s: memset", fn);
  float* NX = sde_noise ? at(o.NX) : nullptr;        // carved last: the ODE layout is that of vv_head_ws_bytes_batch
  if (NX) VV_TRY(vv_head_sde_proj_fused(h, sde_noise, ld_sde, n_steps, B, NX, s));
  // step-invariant work: cond_proj on all rows, silu(cond_proj(cond) + t_emb(t_i)) as bf16 rows [step][2 B], every adaLN modulation
  vv_lin_args a = lin_base(cond, ld_cond, R2, h->cond_proj, D, h->cond_dim, h->wdt, c0, D);
  VV_TRY(vv_linear_ws(&a, nullptr, nullptr, rpart, rpart_n, rtick, rtick_n, stream, nullptr, nullptr, fragq));   // no companion, no copy: bf16 rows; fragq only for the profiler's record
  VV_TRY(vv_add_rows_silu_bf16(c0, D, temb, D, c, (int)R, R2, D, stream));
  VV_TRY(head_modulations(h, c, (int)R, mod, modf, true, true, stream));
  for (int b = 0; b < B; ++b)
    VV_TRY(vv_head_init_fused(h, noise + (size_t)b * ld_noise, Xs + (size_t)b * sst, Ms + (size_t)b * sst, hb[0] + (size_t)2 * b * D, D, s));
  for (int i = 0; i < n_steps; ++i) {
    float* hc = hb[i & 1];
    for (int l = 0; l < h->layers; ++l) {
      const vv_head_layer& L = h->layer[l];
      const float* ml = mod[l] + (size_t)R2 * i * 3 * D;
      a = lin_base(hc, D, R2, L.wgate, h->ffn, D, h->wdt, act, h->ffn);
      a.pro = VV_PRO_RMSNORM; a.norm_w = L.norm_w; a.eps = h->eps;
      a.mod_shift = ml; a.mod_scale = ml + D; a.ld_mod = 3 * D;
      a.w2 = L.wup; a.act = VV_ACT_SWIGLU; a.flags = VV_LIN_W_REUSED;
      VV_TRY(vv_linear_ws(&a, L.f_gate, L.f_up, rpart, rpart_n, rtick, rtick_n, stream, f8q ? &L.q_gate : nullptr, f8q ? &L.q_up : nullptr, fragq));
      a = lin_base(act, h->ffn, R2, L.wdown, D, h->ffn, h->wdt, hc, D);
      a.gate = ml + 2 * D; a.gate_ld = 3 * D; a.res = hc; a.ldres = D; a.flags = VV_LIN_W_REUSED;
      VV_TRY(vv_linear_ws(&a, L.f_down, nullptr, rpart, rpart_n, rtick, rtick_n, stream, f8q ? &L.q_down : nullptr, nullptr, fragq));
    }
    const float* mf = modf + (size_t)R2 * i * 2 * D;
    VV_TRY(vv_head_boundary_batch(h, hc, D, mf, mf + D, 2 * D, cfg_scale, &coef[i], Xs, Ms, sst, hb[(i + 1) & 1], D, latent_out, ld_latent, B, s,
                                  NX ? NX + (size_t)i * sst : nullptr, (int64_t)n_steps * sst, cfg_rows));
  }
  return 0;
}

extern "C" int vv_head_sample_batch(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                                    const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, int64_t ld_latent, int B, void* ws,
                                    vv_stream_t stream) {
  return head_sample_batch(nullptr, h, cond, ld_cond, noise, ld_noise, temb, coef, n_steps, cfg_scale, latent_out, ld_latent, B, ws,
                           nullptr, 0, stream);
}

extern "C" int vv_head_sample_batch_sde(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                                        const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, int64_t ld_latent, int B, void* ws,
                                        const float* sde_noise, int64_t ld_sde, vv_stream_t stream) {
  return head_sample_batch("vv_head_sample_batch_sde", h, cond, ld_cond, noise, ld_noise, temb, coef, n_steps, cfg_scale, latent_out, ld_latent, B, ws,
                           sde_noise, ld_sde, stream);
}

// guidance per utterance: cfg_rows[B] on the device, read by the solver boundary's blocks (the only place the batched sampler reads the scale);
// every other launch is vv_head_sample_batch's (sde_noise == NULL) or vv_head_sample_batch_sde's
extern "C" int vv_head_sample_batch_cfg(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                                        const vv_dpm_coef* coef, int n_steps, const float* cfg_rows, float* latent_out, int64_t ld_latent, int B, void* ws,
                                        const float* sde_noise, int64_t ld_sde, vv_stream_t stream) {
  if (!cfg_rows) return vv_set_error(VV_E_ARG, "vv_head_sample_batch_cfg: null cfg_rows");
  return head_sample_batch("vv_head_sample_batch_cfg", h, cond, ld_cond, noise, ld_noise, temb, coef, n_steps, 0.f, latent_out, ld_latent, B, ws,
                           sde_noise, ld_sde, stream, cfg_rows);
}

// ---------------------------------------------------------------------------------------------------------------
// causal conv tokenizer (decoder / encoder)
// ---------------------------------------------------------------------------------------------------------------
static inline int conv_ctx_of(const vv_conv& c) { return c.transposed ? 1 : c.kk - c.stride; }

// max floats any [rows, C] activation (incl. left context and right padding) can take for an input of t_in steps
static void convnet_sizes(const vv_convnet* net, int64_t t_in, int decoder, size_t* act_elems, size_t* hid_elems) {
  size_t amax = 0, hmax = 0;
  int64_t T = t_in;
  for (int i = 0; i < net->n_stages; ++i) {
    const vv_conv& cv = net->sample[i];
    const int ctx = conv_ctx_of(cv);
    size_t in_el = (size_t)(T + ctx + cv.kk + cv.stride) * cv.cin;   // generous right padding for ragged tails
    if (in_el > amax) amax = in_el;
    if (cv.transposed) T = T * cv.stride; else T = (T + cv.stride - 1) / cv.stride;
    const size_t C = cv.cout;
    size_t el = (size_t)(T + 8) * C;
    if (el > amax) amax = el;
    if (net->n_blocks[i] > 0 && (size_t)T * 4 * C > hmax) hmax = (size_t)T * 4 * C;
  }
  size_t in_el = (size_t)(T + 8 + net->head.kk) * net->head.cin;
  if (in_el > amax) amax = in_el;
  (void)decoder;
  *act_elems = amax + 64;
  *hid_elems = hmax + 64;
}

// streaming nets (every conv carries a state buffer): each conv's padded input [ctx + T, cin] gets a region of its own, so the left
// contexts of ALL convs can be put in place by one launch before the first conv runs and collected by one launch after the last
static bool convnet_streaming(const vv_convnet* net) {
  for (int i = 0; i <= net->n_stages; ++i) {
    const vv_conv& cv = (i == net->n_stages) ? net->head : net->sample[i];
    if (conv_ctx_of(cv) > 0 && !cv.state) return false;
  }
  return true;
}
static size_t convnet_pad_floats(const vv_convnet* net, int64_t t_in, size_t* offs /* [n_stages + 1] or null */) {
  size_t tot = 0;
  int64_t T = t_in;
  for (int i = 0; i <= net->n_stages; ++i) {
    const vv_conv& cv = (i == net->n_stages) ? net->head : net->sample[i];
    if (offs) offs[i] = tot;
    tot += (((size_t)(T + conv_ctx_of(cv) + 2) * cv.cin) + 63) & ~(size_t)63;
    if (cv.transposed) T = T * cv.stride; else T = (T + cv.stride - 1) / cv.stride;
  }
  return tot;
}

// scratch histories of the one-row stage's blocks (<= 16 blocks x 6 rows x 2048 channels), see run_blocks
#define VV_ROW_BLOCKS 16
#define VV_ROW_HIST_FLOATS ((size_t)VV_ROW_BLOCKS * 6 * 2048)
#define VV_CTX_ITEMS (VV_MAX_STAGES + 1 + 16)   // capacity of a net's streaming-state move list (= vv_conv_ctx_batch's limit, vv_fused.hip)

extern "C" size_t vv_convnet_ws_bytes(const vv_convnet* net, int64_t t_in, int decoder) {
  if (!net || t_in <= 0) return 0;
  VV_WQ_STRIP(vv_convnet, net);
  size_t a, h;
  convnet_sizes(net, t_in, decoder, &a, &h);
  return 2 * al(a) + al(h) + (convnet_streaming(net) ? al(convnet_pad_floats(net, t_in, nullptr)) + al(VV_ROW_HIST_FLOATS) : 0);
}

// Runs the stage's blocks on the ping-pong buffers cur / other.  The LAST block writes its result `nctx` rows into a buffer so
// that it becomes the next conv's padded input; *pad_out is that buffer.  Unfused block (mixer -> other, lin1 -> hid, lin2): the
// dead input buffer is the only one free, so the result goes there, shifted.  Fused block (one launch reads its input while
// other row tiles already write): the result must not overlap the input; `other` is free (no mixer output) and takes it.
static int run_blocks(const vv_convnet* net, int wq, int stage, int64_t T, int C, float*& cur, float*& other, float* hid,
                      int nctx, float** pad_out, vv_stream_t stream, float* next_pad = nullptr, float* row_hist = nullptr,
                      vv_conv_ctx_item* items = nullptr, int* n_items = nullptr, int* row_stage = nullptr) {
  // row_hist / items (streaming nets): scratch for the new histories of the one-row stage's blocks and the list of state moves that the
  // net's closing vv_conv_ctx_batch performs (a block's history may only be replaced once every workgroup that reads it is done)
  // next_pad (streaming nets): the next conv's own padded-input region; the stage result goes to next_pad + nctx rows
  const int nb = net->n_blocks[stage];
  for (int j = 0; j < nb; ++j) {
    const vv_block& B = net->blocks[stage][j];
    const bool last = (j == nb - 1);
    if (!vv_convffn_prefers(net->wdt, (int)T, C)) {   // narrow stages with many rows: the whole block as one launch (vv_block1d.hip)
      float* dst = last ? (next_pad ? next_pad : other) + (size_t)nctx * C : other;
      const int fused = vv_launch_block1d(B, net->wdt, cur, dst, (int)T, C, net->eps, (hipStream_t)stream);
      if (fused < 0) return fused;
      if (fused) {
        if (last) { *pad_out = next_pad ? next_pad : other; cur = nullptr; }
        else { float* t = cur; cur = other; other = t; }
        continue;
      }
    }
    float* final_dst = last ? (next_pad ? next_pad : cur) + (size_t)nctx * C : nullptr;
    if (last) *pad_out = next_pad ? next_pad : cur;
    // one-row fast path: row_hist holds one scratch history per block index j, so only ONE stage of a net may take it (the shipped nets
    // have a single T == 1 stage; a second one falls through to the general path below), and the item list must have room
    if (T == 1 && row_hist && items && n_items && j < VV_ROW_BLOCKS && B.hist && !B.q_w1.q && *n_items < VV_CTX_ITEMS &&
        (*row_stage < 0 || *row_stage == stage)) {
      // the one-row stage (C = 2048): mixer + RMSNorm + first GEMM + GELU as one launch (vv_convffn.hip), then the weight-streaming GEMV
      float* hn = row_hist + (size_t)j * 6 * C;
      int one = vv_launch_ffn_in_row_hs(B, net->wdt, cur, other, hid, hn, C, net->eps, (hipStream_t)stream);
      if (one == 0) one = vv_launch_ffn_in_row(B, net->wdt, cur, other, hid, hn, C, net->eps, (hipStream_t)stream);
      if (one < 0) return one;
      if (one) {
        *row_stage = stage;
        items[(*n_items)++] = vv_conv_ctx_item{hn, B.hist, 6, 0, C, B.dw_w, B.hs};   // the scatter also refreshes hs from the rows it stores
        float* dst1 = (last && final_dst) ? final_dst : other;
        vv_lin_args a1 = lin_base(hid, 4 * C, 1, B.w2, C, 4 * C, net->wdt, dst1, C);
        a1.bias = B.b2; a1.gate = B.ffn_gamma; a1.gate_ld = 0; a1.res = other; a1.ldres = C;
        use_w8(a1, wq, B.q_w2);
        VV_TRY(vv_linear(&a1, stream));
        if (dst1 == other) { float* t = cur; cur = other; other = t; }
        else { cur = nullptr; }
        continue;
      }
    }
    if (B.hs && B.hist && items && n_items) {
      if (*n_items >= VV_CTX_ITEMS) return vv_set_error(VV_E_UNSUPPORTED, "convnet: more than %d streaming-state moves in one net", VV_CTX_ITEMS);
      items[(*n_items)++] = vv_conv_ctx_item{B.hist, B.hist, 6, 0, C, B.dw_w, B.hs};   // this block's history changes below on a general path: hs follows at the closing scatter
    }
    {   // middle stages of a streaming frame (C = 256 / 512): mixer + first GEMM, second GEMM (vv_convffn.hip); the bf16 hidden tile
        // fills the first half of `hid`, the scratch history sits behind it
      float* dst2 = (last && final_dst) ? final_dst : other;
      const int two = vv_launch_convffn(B, net->wdt, cur, other, hid, reinterpret_cast<float*>(reinterpret_cast<char*>(hid) + (size_t)T * 4 * C * 2),
                                        dst2, (int)T, C, net->eps, (hipStream_t)stream);
      if (two < 0) return two;
      if (two) {
        if (dst2 == other) { float* t = cur; cur = other; other = t; }
        else { cur = nullptr; }
        continue;
      }
    }
    VV_TRY(vv_block_mixer(cur, other, (int)T, C, B.norm_w, net->eps, B.dw_w, B.dw_b, B.gamma, B.hist, stream));
    // T > 8 rows on bf16 weights: both FFN linears run on the matrix cores and the 4C-wide hidden activation is handed
    // over in bf16 (half the bytes, and the second GEMM reads its fragments straight from it: no LDS staging)
    const bool handoff = net->wdt == VV_BF16 && T > 8 && C % 16 == 0 && ((uintptr_t)B.w1 % 16 == 0) && ((uintptr_t)B.w2 % 16 == 0);
    vv_lin_args a;
    const long tiles1 = (long)((4 * C) / 128) * ((T + 127) / 128);   // 128 x 128 output tiles of the first FFN GEMM
    if (handoff && C % 32 == 0 && (4 * C) % 128 == 0 && T >= 64 && tiles1 >= 24) {
      // whole-utterance sequences (enough output tiles for the LDS-tiled 128 x 128 kernel; a streaming frame never has them):
      // RMSNorm + bf16 cast once, then both FFN GEMMs stream bf16 activations.  The cast rows live in the half of `hid`
      // that the bf16 hidden tile leaves free.
      void* xb = reinterpret_cast<char*>(hid) + (size_t)T * 4 * C * 2;
      VV_TRY(vv_cast_rows_bf16(other, C, (int)T, C, VV_PRO_RMSNORM, B.ffn_norm_w, net->eps, xb, C, stream));
      a = lin_base((const float*)xb, C, (int)T, B.w1, 4 * C, C, net->wdt, hid, 4 * C);
      a.flags = VV_LIN_X_BF16; a.bias = B.b1; a.act = VV_ACT_GELU;
    } else {
      a = lin_base(other, C, (int)T, B.w1, 4 * C, C, net->wdt, hid, 4 * C);
      a.pro = VV_PRO_RMSNORM; a.norm_w = B.ffn_norm_w; a.eps = net->eps; a.bias = B.b1; a.act = VV_ACT_GELU;
    }
    if (handoff) a.flags |= VV_LIN_OUT_BF16;
    use_w8(a, wq, B.q_w1);
    VV_TRY(vv_linear(&a, stream));
    float* dst = (j == nb - 1 && final_dst) ? final_dst : other;
    a = lin_base(hid, 4 * C, (int)T, B.w2, C, 4 * C, net->wdt, dst, C);
    if (handoff) a.flags |= VV_LIN_X_BF16;
    a.bias = B.b2; a.gate = B.ffn_gamma; a.gate_ld = 0; a.res = other; a.ldres = C;
    use_w8(a, wq, B.q_w2);
    VV_TRY(vv_linear(&a, stream));
    if (dst == other) { float* t = cur; cur = other; other = t; }   // result now in `cur`
    else { cur = nullptr; }                                           // result went to final_dst
  }
  return 0;
}

// prepare the left context of a conv's padded input buffer `pad` (= [ctx rows | T rows already written by the producer])
static int conv_left_ctx(const vv_conv& cv, float* pad, int64_t T, vv_stream_t stream) {
  const int ctx = conv_ctx_of(cv);
  if (ctx <= 0) return 0;
  if (cv.state) return vv_conv_ctx(pad, cv.state, ctx, (int)T, cv.cin, stream);
  hipError_t e = hipMemsetAsync(pad, 0, (size_t)ctx * cv.cin * 4, (hipStream_t)stream);
  if (e != hipSuccess) return vv_set_error(VV_E_HIP, "conv_left_ctx: %s", hipGetErrorString(e));
  return 0;
}

// vv_decoder_forward, and - mid != NULL - vv_decoder_forward_from: the frame enters behind the hand-over conv (sample[1]) with mid = that conv's
// output [stride, cout]; stage 0, the hand-over conv and their streaming state are the caller's (vv_decoder_front_rows)
static int decoder_run(const char* who, const vv_convnet* net, const float* latent, int T0, float pre_scale, float pre_bias, float* wav,
                       void* ws, vv_stream_t stream, const float* mid) {
  if (!net || (!latent && !mid) || !wav || !ws) return vv_set_error(VV_E_ARG, "%s: null pointer", who);
  if (T0 <= 0 || net->n_stages < 1 || net->n_stages > VV_MAX_STAGES) return vv_set_error(VV_E_ARG, "%s: bad T/stages", who);
  VV_WQ_STRIP(vv_convnet, net);
  const int first = mid ? 1 : 0;                  // the first stage this call runs
  size_t ael, hel;
  convnet_sizes(net, T0, 1, &ael, &hel);
  Carver cvr(ws);
  float* A = cvr.take(ael);
  float* Bf = cvr.take(ael);
  float* hid = cvr.take(hel);
  int64_t T = T0;
  // stem input: padded [6 + T, vae] in A
  const vv_conv& stem = net->sample[0];
  if (stem.transposed || stem.stride != 1) return vv_set_error(VV_E_ARG, "%s: stem must be a stride-1 conv", who);
  // streaming: every conv reads its own padded-input region; all left contexts are placed by ONE launch up front and collected by
  // ONE launch at the end (they were one dependent launch per conv: 8 per frame and net)
  const bool streaming = convnet_streaming(net);
  if (mid && (!streaming || net->n_stages < 2 || !net->sample[1].transposed))
    return vv_set_error(VV_E_UNSUPPORTED, "%s: needs a streaming net whose second conv is the transposed hand-over", who);
  size_t poff[VV_MAX_STAGES + 1];
  float* pads = nullptr;
  vv_conv_ctx_item items[VV_CTX_ITEMS];
  int n_items = 0, row_stage = -1;
  float* row_hist = nullptr;
  if (streaming) {
    pads = cvr.take(convnet_pad_floats(net, T0, poff));
    row_hist = cvr.take(VV_ROW_HIST_FLOATS);
    int64_t Ti = T0;
    for (int i = 0; i <= net->n_stages; ++i) {
      const vv_conv& cv = (i == net->n_stages) ? net->head : net->sample[i];
      if (conv_ctx_of(cv) > 0 && (!mid || i > 1)) items[n_items++] = vv_conv_ctx_item{pads + poff[i], cv.state, conv_ctx_of(cv), (int)Ti, cv.cin};
      if (cv.transposed) Ti *= cv.stride;
    }
    // the scaled latent frame rides along with the context gather: one launch instead of two in front of the stem conv
    vv_conv_ctx_item gi[VV_MAX_STAGES + 2];
    for (int i = 0; i < n_items; ++i) gi[i] = items[i];
    int n_gather = n_items;
    if (!mid)
      gi[n_gather++] = vv_conv_ctx_item{pads + poff[0] + (size_t)conv_ctx_of(stem) * stem.cin, const_cast<float*>(latent), (int)T, 0, stem.cin, nullptr, nullptr, 1,
                                        pre_scale, pre_bias};
    VV_TRY(vv_conv_ctx_batch(gi, n_gather, 0, (hipStream_t)stream));
  }
  float* pad = streaming ? pads + poff[0] : A;
  if (!streaming) VV_TRY(vv_affine(latent, pre_scale, pre_bias, pad + (size_t)conv_ctx_of(stem) * stem.cin, (int64_t)T * stem.cin, stream));
  float* cur = nullptr;     // current activation buffer, `pad` holds the next conv's input
  float* other = nullptr;
  for (int i = first; i < net->n_stages; ++i) {
    const vv_conv& cv = net->sample[i];
    if (!streaming) VV_TRY(conv_left_ctx(cv, pad, T, stream));
    float* outb = (pad == A) ? Bf : A;
    vv_lin_args a;
    if (mid && i == 1) {        // the hand-over conv ran in the caller: its output rows become this stage's input (the blocks ping-pong on A / Bf)
      outb = A;
      T *= cv.stride;
      hipError_t e = hipMemcpyAsync(outb, mid, (size_t)T * cv.cout * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
      if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
    } else if (cv.transposed) {
      a = lin_base(pad, cv.cin, (int)T, cv.w, cv.stride * cv.cout, 2 * cv.cin, net->wdt, outb, (int64_t)cv.stride * cv.cout);
      a.bias = cv.b;
      VV_TRY(vv_linear(&a, stream));
      T *= cv.stride;
    } else {
      a = lin_base(pad, (int64_t)cv.stride * cv.cin, (int)T, cv.w, cv.cout, cv.kk * cv.cin, net->wdt, outb, cv.cout);
      a.bias = cv.b;
      VV_TRY(vv_linear(&a, stream));
    }
    cur = outb;
    other = (cur == A) ? Bf : A;
    const int C = cv.cout;
    const vv_conv& nxt = (i + 1 < net->n_stages) ? net->sample[i + 1] : net->head;
    const int nctx = conv_ctx_of(nxt);
    float* next_pad = streaming ? pads + poff[i + 1] : nullptr;
    if (net->n_blocks[i] > 0) {
      // the last block writes straight into the next conv's padded input; which buffer that is depends on block parity:
      // block j reads cur -> writes other, then they swap.  The last block's mixer output sits in `other_last`, its
      // result may go anywhere except that buffer and hid: use the buffer holding the (dead) input of that block.
      VV_TRY(run_blocks(net, wq, i, T, C, cur, other, hid, nctx, &pad, stream, next_pad, row_hist, items, &n_items, &row_stage));
    } else {
      float* dstb = next_pad ? next_pad : other;
      hipError_t e = hipMemcpyAsync(dstb + (size_t)nctx * C, cur, (size_t)T * C * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream);
      if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
      pad = dstb;
    }
  }
  const vv_conv& hd = net->head;
  if (!streaming) VV_TRY(conv_left_ctx(hd, pad, T, stream));
  vv_lin_args a = lin_base(pad, (int64_t)hd.stride * hd.cin, (int)T, hd.w, hd.cout, hd.kk * hd.cin, net->wdt, wav, hd.cout);
  a.bias = hd.b;
  VV_TRY(vv_linear(&a, stream));
  if (streaming) VV_TRY(vv_conv_ctx_batch(items, n_items, 1, (hipStream_t)stream));
  return 0;
}

extern "C" int vv_decoder_forward(const vv_convnet* net, const float* latent, int T0, float pre_scale, float pre_bias, float* wav,
                                  void* ws, vv_stream_t stream) {
  if (!latent) return vv_set_error(VV_E_ARG, "vv_decoder_forward: null pointer");
  return decoder_run("vv_decoder_forward", net, latent, T0, pre_scale, pre_bias, wav, ws, stream, nullptr);
}

extern "C" int vv_decoder_forward_from(const vv_convnet* net, const float* mid, float* wav, void* ws, vv_stream_t stream) {
  if (!mid) return vv_set_error(VV_E_ARG, "vv_decoder_forward_from: null pointer");
  return decoder_run("vv_decoder_forward_from", net, nullptr, 1, 0.f, 0.f, wav, ws, stream, mid);
}

// vv_encoder_forward, and - mid_out != NULL - vv_encoder_forward_until: the frame leaves behind the blocks of the last stage but one, whose result
// goes to mid_out [T, C] instead of the hand-over conv's padded input; that conv, the last stage, the head and their state are the caller's
// (vv_encoder_back_rows)
static int encoder_run(const char* who, const vv_convnet* net, const float* wav, int64_t T0, float* feat, void* ws, vv_stream_t stream, float* mid_out) {
  if (!net || !wav || (!feat && !mid_out) || !ws) return vv_set_error(VV_E_ARG, "%s: null pointer", who);
  if (T0 <= 0 || net->n_stages < 1 || net->n_stages > VV_MAX_STAGES) return vv_set_error(VV_E_ARG, "%s: bad T/stages", who);
  VV_WQ_STRIP(vv_convnet, net);
  const int last_i = mid_out ? net->n_stages - 2 : net->n_stages;      // the last conv this call runs (n_stages: the head)
  hipStream_t s = (hipStream_t)stream;
  size_t ael, hel;
  convnet_sizes(net, T0, 0, &ael, &hel);
  Carver cvr(ws);
  float* A = cvr.take(ael);
  float* Bf = cvr.take(ael);
  float* hid = cvr.take(hel);
  int64_t T = T0;
  const vv_conv& stem = net->sample[0];
  // streaming frames (T0 a multiple of the hop, every conv with a state buffer): dedicated padded-input regions, all left contexts
  // gathered / scattered by one launch each (see vv_decoder_forward)
  bool streaming = convnet_streaming(net);
  {
    int64_t Ti = T0;
    for (int i = 0; i < net->n_stages && streaming; ++i) { if (Ti % net->sample[i].stride) streaming = false; Ti /= net->sample[i].stride; }
  }
  if (mid_out && (!streaming || net->n_stages < 2)) return vv_set_error(VV_E_UNSUPPORTED, "%s: needs a streaming frame of a net with two stages or more", who);
  size_t poff[VV_MAX_STAGES + 1];
  float* pads = nullptr;
  vv_conv_ctx_item items[VV_CTX_ITEMS];
  int n_items = 0, row_stage = -1;
  float* row_hist = nullptr;
  if (streaming) {
    pads = cvr.take(convnet_pad_floats(net, T0, poff));
    row_hist = cvr.take(VV_ROW_HIST_FLOATS);
    int64_t Ti = T0;
    for (int i = 0; i <= net->n_stages; ++i) {
      const vv_conv& cv = (i == net->n_stages) ? net->head : net->sample[i];
      if (conv_ctx_of(cv) > 0 && i <= last_i) items[n_items++] = vv_conv_ctx_item{pads + poff[i], cv.state, conv_ctx_of(cv), (int)Ti, cv.cin};
      Ti = (Ti + cv.stride - 1) / cv.stride;
    }
    // the waveform chunk rides along with the context gather (no separate copy in front of the stem conv)
    vv_conv_ctx_item gi[VV_MAX_STAGES + 2];
    for (int i = 0; i < n_items; ++i) gi[i] = items[i];
    gi[n_items] = vv_conv_ctx_item{pads + poff[0] + (size_t)conv_ctx_of(stem) * stem.cin, const_cast<float*>(wav), (int)T, 0, stem.cin, nullptr, nullptr, 1, 1.0f, 0.0f};
    VV_TRY(vv_conv_ctx_batch(gi, n_items + 1, 0, s));
  }
  float* pad = streaming ? pads + poff[0] : A;
  hipError_t e = hipSuccess;
  if (!streaming) e = hipMemcpyAsync(pad + (size_t)conv_ctx_of(stem) * stem.cin, wav, (size_t)T * stem.cin * 4, hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
  float* cur = nullptr;
  float* other = nullptr;
  for (int i = 0; i <= last_i; ++i) {
    const bool is_head = (i == net->n_stages);
    const vv_conv& cv = is_head ? net->head : net->sample[i];
    if (cv.transposed) return vv_set_error(VV_E_ARG, "%s: transposed conv in an encoder", who);
    const int ctx = conv_ctx_of(cv);
    if (!streaming) VV_TRY(conv_left_ctx(cv, pad, T, stream));
    // output length as the reference's non-streaming padding rule gives it (modular_vibevoice_tokenizer.py:127-133);
    // for streaming frames T is a multiple of the stride and there is no tail.
    const int64_t Tout = (T + cv.stride - 1) / cv.stride;
    const int64_t need = (Tout - 1) * cv.stride + cv.kk;        // rows of the padded buffer the conv reads
    const int64_t have = ctx + T;
    if (need > have) {
      e = hipMemsetAsync(pad + (size_t)have * cv.cin, 0, (size_t)(need - have) * cv.cin * 4, s);
      if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    float* outb = is_head ? feat : ((pad == A) ? Bf : A);
    vv_lin_args a = lin_base(pad, (int64_t)cv.stride * cv.cin, (int)Tout, cv.w, cv.cout, cv.kk * cv.cin, net->wdt, outb, cv.cout);
    a.bias = cv.b;
    {   // whole-utterance sequences: the padded input is cast to bf16 once (into `hid`, free between stages) and the conv - a GEMM
        // over overlapping rows - runs on the LDS-tiled kernel; a streaming frame never has the >= 24 output tiles this needs
      const long tiles = (long)(cv.cout / 128) * ((Tout + 127) / 128);
      const size_t in_el = (size_t)need * cv.cin;
      if (net->wdt == VV_BF16 && !is_head && cv.cout % 128 == 0 && (cv.kk * cv.cin) % 32 == 0 && (cv.stride * cv.cin) % 8 == 0 && cv.cin >= 128 && cv.cin % 8 == 0 &&
          tiles >= 24 && in_el * 2 <= hel * 4 && ((uintptr_t)cv.w % 16 == 0)) {
        VV_TRY(vv_cast_rows_bf16(pad, cv.cin, (int)need, cv.cin, VV_PRO_NONE, nullptr, 0.f, hid, cv.cin, stream));
        a.x = hid; a.flags = VV_LIN_X_BF16;
      } else if (net->wdt == VV_BF16 && is_head && Tout >= 64 && cv.cout % 64 == 0 && (cv.kk * cv.cin) % 128 == 0 && cv.kk * cv.cin >= 8192 &&
                 (cv.stride * cv.cin) % 8 == 0 && cv.cin % 8 == 0 && in_el * 2 <= hel * 4 && ((uintptr_t)cv.w % 16 == 0)) {
        // the head conv of a long sequence (few output channels, K = 7 x 2048): same cast, 64 x 64 tiles over the long K
        VV_TRY(vv_cast_rows_bf16(pad, cv.cin, (int)need, cv.cin, VV_PRO_NONE, nullptr, 0.f, hid, cv.cin, stream));
        a.x = hid; a.flags = VV_LIN_X_BF16;
      }
    }
    VV_TRY(vv_linear(&a, stream));
    if (is_head) break;
    T = Tout;
    cur = outb;
    other = (cur == A) ? Bf : A;
    const int C = cv.cout;
    const vv_conv& nxt = (i + 1 < net->n_stages) ? net->sample[i + 1] : net->head;
    const bool leave = mid_out && i == last_i;                      // this stage's result is the call's output
    const int nctx = leave ? 0 : conv_ctx_of(nxt);
    float* next_pad = leave ? mid_out : streaming ? pads + poff[i + 1] : nullptr;
    if (net->n_blocks[i] > 0) {
      VV_TRY(run_blocks(net, wq, i, T, C, cur, other, hid, nctx, &pad, stream, next_pad, row_hist, items, &n_items, &row_stage));
    } else {
      float* dstb = next_pad ? next_pad : other;
      e = hipMemcpyAsync(dstb + (size_t)nctx * C, cur, (size_t)T * C * 4, hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", who, hipGetErrorString(e));
      pad = dstb;
    }
  }
  if (streaming) VV_TRY(vv_conv_ctx_batch(items, n_items, 1, s));
  return 0;
}

extern "C" int vv_encoder_forward(const vv_convnet* net, const float* wav, int64_t T0, float* feat, void* ws, vv_stream_t stream) {
  if (!feat) return vv_set_error(VV_E_ARG, "vv_encoder_forward: null pointer");
  return encoder_run("vv_encoder_forward", net, wav, T0, feat, ws, stream, nullptr);
}

extern "C" int vv_encoder_forward_until(const vv_convnet* net, const float* wav, int64_t T, float* mid, void* ws, vv_stream_t stream) {
  if (!mid) return vv_set_error(VV_E_ARG, "vv_encoder_forward_until: null pointer");
  return encoder_run("vv_encoder_forward_until", net, wav, T, nullptr, ws, stream, mid);
}

extern "C" int vv_convnet_reset(const vv_convnet* net, vv_stream_t stream) {
  if (!net) return vv_set_error(VV_E_ARG, "vv_convnet_reset: null");
  VV_WQ_STRIP(vv_convnet, net);
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i <= net->n_stages; ++i) {
    const vv_conv& cv = (i == net->n_stages) ? net->head : net->sample[i];
    if (cv.state) {
      hipError_t e = hipMemsetAsync(cv.state, 0, (size_t)conv_ctx_of(cv) * cv.cin * 4, s);
      if (e != hipSuccess) return vv_set_error(VV_E_HIP, "vv_convnet_reset: %s", hipGetErrorString(e));
    }
    if (i < net->n_stages) {
      for (int j = 0; j < net->n_blocks[i]; ++j) {
        const vv_block& B = net->blocks[i][j];
        if (B.hist) {
          hipError_t e = hipMemsetAsync(B.hist, 0, (size_t)6 * net->sample[i].cout * 4, s);
          if (e != hipSuccess) return vv_set_error(VV_E_HIP, "vv_convnet_reset: %s", hipGetErrorString(e));
        }
        if (B.hs) {
          hipError_t e = hipMemsetAsync(B.hs, 0, (size_t)net->sample[i].cout * 4, s);
          if (e != hipSuccess) return vv_set_error(VV_E_HIP, "vv_convnet_reset: %s", hipGetErrorString(e));
        }
      }
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// the one-row stage (C = 2048, one row per frame) of both tokenizers for the B dialogues of a row batch: one pass over its weights
// (kernels: vv_conv_hot.hip).  The dialogues' nets are forks of one net - same weights, every state pointer moved by one offset per dialogue.
// ---------------------------------------------------------------------------------------------------------------
namespace {

struct RowsPlan {
  vv_convnet net;          // dialogue 0's net, wdt stripped
  vv_rows_delta dl;        // dialogue b's state = dialogue 0's + dl.d[b] floats
  int rs;                  // the one-row stage
  int nb;                  // its blocks
  const vv_conv* ho;       // the hand-over conv between it and the C = 1024 stage
  int ctx0, P0;            // decoder: the stem's left context rows and the pitch of a dialogue's padded stem input
  int ctxh, Kh;            // the hand-over conv's left context rows and its K (= pitch of a dialogue's padded input)
  int ctxd, PH;            // encoder: the head conv's left context rows and the pitch of a dialogue's padded head input
};

inline int r64(size_t n) { return (int)((n + 63) & ~(size_t)63); }

// the shape part of the coverage: net alone (vv_conv_rows_ws_bytes asks with one net)
int rows_shape(const char* who, const vv_convnet* net0, int decoder, RowsPlan* p) {
  p->net = *net0;
  vv_convnet& n = p->net;
  if (n.wdt & vv_wq_bits()) return vv_set_error(VV_E_UNSUPPORTED, "%s: quantised companions are not served", who);
  if (n.wdt != VV_BF16) return vv_set_error(VV_E_UNSUPPORTED, "%s: bf16 weights only", who);
  if (n.n_stages < 2 || n.n_stages > VV_MAX_STAGES) return vv_set_error(VV_E_UNSUPPORTED, "%s: %d stages", who, n.n_stages);
  if (!convnet_streaming(&n)) return vv_set_error(VV_E_UNSUPPORTED, "%s: a streaming net (every conv with its state) only", who);
  p->rs = decoder ? 0 : n.n_stages - 1;
  p->nb = n.n_blocks[p->rs];
  p->ho = decoder ? &n.sample[1] : &n.sample[n.n_stages - 1];
  const vv_conv& ho = *p->ho;
  if (n.sample[p->rs].cout != 2048 || p->nb < 1 || p->nb > VV_ROW_BLOCKS || p->nb + 4 > VV_ROWS_ITEMS)
    return vv_set_error(VV_E_UNSUPPORTED, "%s: the one-row stage must be C = 2048 with 1..%d blocks (C = %d, %d blocks)", who, VV_ROW_BLOCKS, n.sample[p->rs].cout, p->nb);
  for (int j = 0; j < p->nb; ++j) {
    const vv_block& b = n.blocks[p->rs][j];
    if (b.q_w1.q || b.q_w2.q) return vv_set_error(VV_E_UNSUPPORTED, "%s: fp8 companions are not served", who);
    if (!b.hist || !b.hs || !b.dw_last) return vv_set_error(VV_E_UNSUPPORTED, "%s: the one-row blocks need hist, hs and dw_last", who);
  }
  if (decoder) {
    const vv_conv& stem = n.sample[0];
    if (stem.transposed || stem.stride != 1 || !ho.transposed || ho.cin != 2048 || ho.stride * ho.cout != 8192)
      return vv_set_error(VV_E_UNSUPPORTED, "%s: needs a stride-1 stem and the transposed hand-over 2048 -> 8 x 1024", who);
    p->ctx0 = conv_ctx_of(stem); p->P0 = r64((size_t)(p->ctx0 + 3) * stem.cin);
    p->ctxh = 1; p->Kh = 2 * ho.cin;
    p->ctxd = 0; p->PH = 0;
  } else {
    const vv_conv& hd = n.head;
    if (ho.transposed || ho.kk * ho.cin != 16384 || ho.cout != 2048 || ho.kk <= ho.stride || hd.transposed || hd.stride != 1 || hd.cin != 2048)
      return vv_set_error(VV_E_UNSUPPORTED, "%s: needs the strided hand-over with K = 16384 into C = 2048 and a stride-1 head", who);
    p->ctx0 = 0; p->P0 = 0;
    p->ctxh = conv_ctx_of(ho); p->Kh = ho.kk * ho.cin;
    p->ctxd = conv_ctx_of(hd); p->PH = r64((size_t)(p->ctxd + 3) * hd.cin);
  }
  return 0;
}

// nets[0 .. B): forks of one net?  Same weights (VV_E_ARG otherwise), every state pointer of the part these calls run moved by ONE offset per dialogue
int rows_plan(const char* who, const vv_convnet* const* nets, int B, int decoder, RowsPlan* p) {
  if (B < 2 || B > 8) return vv_set_error(VV_E_UNSUPPORTED, "%s: B=%d (2..8 dialogues)", who, B);
  for (int b = 0; b < B; ++b)
    if (!nets[b]) return vv_set_error(VV_E_ARG, "%s: null net", who);
  VV_TRY(rows_shape(who, nets[0], decoder, p));
  const vv_convnet& n0 = p->net;
  const int rs = p->rs, hoi = decoder ? 1 : n0.n_stages - 1;
  const float* base0 = n0.blocks[rs][0].hist;
  p->dl.d[0] = 0;
  for (int b = 1; b < 8; ++b) p->dl.d[b] = 0;
  for (int b = 1; b < B; ++b) {
    const vv_convnet& n = *nets[b];
    if (n.wdt != nets[0]->wdt || n.n_stages != n0.n_stages || n.eps != n0.eps || n.n_blocks[rs] != p->nb || !n.blocks[rs])
      return vv_set_error(VV_E_ARG, "%s: net %d is not a fork of net 0", who, b);
    const int64_t d = n.blocks[rs][0].hist - base0;
    for (int c = 0; c < b; ++c)
      if (d == p->dl.d[c]) return vv_set_error(VV_E_ARG, "%s: nets %d and %d share their streaming state", who, c, b);
    p->dl.d[b] = d;
    auto conv_ok = [&](const vv_conv& a, const vv_conv& f) {
      return a.w == f.w && a.b == f.b && a.cin == f.cin && a.cout == f.cout && a.kk == f.kk && a.stride == f.stride && a.transposed == f.transposed &&
             (a.state ? f.state == a.state + d : !f.state);
    };
    bool ok = conv_ok(n0.sample[rs], n.sample[rs]) && conv_ok(n0.sample[hoi], n.sample[hoi]) && (decoder || conv_ok(n0.head, n.head));
    for (int j = 0; ok && j < p->nb; ++j) {
      const vv_block& a = n0.blocks[rs][j];
      const vv_block& f = n.blocks[rs][j];
      ok = a.gamma == f.gamma && a.ffn_gamma == f.ffn_gamma && a.norm_w == f.norm_w && a.ffn_norm_w == f.ffn_norm_w && a.dw_w == f.dw_w && a.dw_b == f.dw_b &&
           a.w1 == f.w1 && a.b1 == f.b1 && a.w2 == f.w2 && a.b2 == f.b2 && a.dw_last == f.dw_last && !f.q_w1.q && !f.q_w2.q && f.hist == a.hist + d &&
           f.hs == a.hs + d;
    }
    if (!ok) return vv_set_error(VV_E_ARG, "%s: net %d is not a fork of net 0 (same weights, state moved by one offset)", who, b);
  }
  return 0;
}

struct RowsWs { float *X, *Y, *hid, *hn, *pad0, *hpad, *hdpad, *feat; };

size_t rows_carve(const RowsPlan& p, int B, int decoder, void* ws, RowsWs* w) {
  const size_t C = 2048;
  Carver cv(ws);
  char* base = cv.p;
  float* X = cv.take(B * C);
  float* Y = cv.take(B * C);
  float* hid = cv.take(B * 4 * C);
  float* hn = cv.take((size_t)p.nb * B * 6 * C);
  float* pad0 = decoder ? cv.take((size_t)B * p.P0) : nullptr;
  float* hpad = cv.take((size_t)B * p.Kh);
  float* hdpad = decoder ? nullptr : cv.take((size_t)B * p.PH);
  float* feat = decoder ? nullptr : cv.take((size_t)B * p.net.head.cout);
  if (w) *w = RowsWs{X, Y, hid, hn, pad0, hpad, hdpad, feat};
  return (size_t)(cv.p - base);
}

// the stage's blocks on x = w.X: row_in_rows + the W2 GEMV per block; the last block's result goes to row b of (dst, ld_dst)
// and the blocks' history moves join the call's closing scatter
int rows_blocks(const RowsPlan& p, int B, const RowsWs& w, const int* active, float* dst, int64_t ld_dst, vv_rows_item* items, int* n_items, hipStream_t s) {
  const int C = 2048;
  float* cur = w.X;
  float* other = w.Y;
  for (int j = 0; j < p.nb; ++j) {
    const vv_block& blk = p.net.blocks[p.rs][j];
    const bool last = j == p.nb - 1;
    float* hn = w.hn + (size_t)j * B * 6 * C;
    VV_TRY(vv_launch_row_in_rows(blk, B, cur, other, w.hid, hn, p.dl, active, p.net.eps, s));
    items[(*n_items)++] = vv_rows_item{hn, (int64_t)6 * C, blk.hist, 0, 1, 6 * C, C, blk.dw_w, blk.hs, 0, 0.f, 0.f};
    // out = y + ffn_gamma (W2 hidden + b2): y sits in `other`, the result replaces it (each element is read and written by one thread)
    VV_TRY(vv_launch_rows_gemv(VV_ROWS_W2, B, w.hid, 4 * C, blk.w2, blk.b2, blk.ffn_gamma, other, C, last ? dst : other, last ? ld_dst : C, nullptr, s));
    float* t = cur; cur = other; other = t;
  }
  return 0;
}

}  // namespace

extern "C" size_t vv_conv_rows_ws_bytes(const vv_convnet* net, int B, int decoder) {
  if (!net || B < 2 || B > 8) return 0;
  RowsPlan p;
  if (rows_shape("vv_conv_rows_ws_bytes", net, decoder, &p)) return 0;
  return rows_carve(p, B, decoder, nullptr, nullptr);
}

extern "C" int vv_decoder_front_rows(const vv_convnet* const* nets, int B, const int* active, const float* latent, int64_t ld_latent, float pre_scale,
                                     float pre_bias, float* mid, int64_t ld_mid, void* ws, vv_stream_t stream) {
  const char* who = "vv_decoder_front_rows";
  if (!nets || !active || !latent || !mid || !ws) return vv_set_error(VV_E_ARG, "%s: null pointer", who);
  RowsPlan p;
  VV_TRY(rows_plan(who, nets, B, 1, &p));
  const vv_conv& stem = p.net.sample[0];
  const vv_conv& ho = *p.ho;
  if (ld_latent < stem.cin || ld_mid < (int64_t)ho.stride * ho.cout || ld_mid % 4 || ((uintptr_t)mid % 16))
    return vv_set_error(VV_E_ARG, "%s: ld_latent=%lld ld_mid=%lld", who, (long long)ld_latent, (long long)ld_mid);
  hipStream_t s = (hipStream_t)stream;
  const int C = 2048;
  RowsWs w;
  rows_carve(p, B, 1, ws, &w);
  const int nin = p.ctx0 * stem.cin;
  vv_rows_item items[VV_ROWS_ITEMS];
  int n = 0;
  // every dialogue's left contexts and its scaled latent frame into place: one launch
  items[n++] = vv_rows_item{w.pad0, p.P0, stem.state, 0, 1, nin, stem.cin, nullptr, nullptr, 0, 0.f, 0.f};
  items[n++] = vv_rows_item{w.pad0 + nin, p.P0, const_cast<float*>(latent), ld_latent, 0, stem.cin, stem.cin, nullptr, nullptr, 1, pre_scale, pre_bias};
  items[n++] = vv_rows_item{w.hpad, p.Kh, ho.state, 0, 1, ho.cin, ho.cin, nullptr, nullptr, 0, 0.f, 0.f};
  VV_TRY(vv_launch_rows_ctx(items, n, B, p.dl, active, 0, s));
  // the stem conv (K = 7 x latent, 1.8 MB) per dialogue as vv_decoder_forward runs it: the one-row blocks' histories then match it bit for bit
  for (int b = 0; b < B; ++b) {
    vv_lin_args a = lin_base(w.pad0 + (size_t)b * p.P0, (int64_t)stem.stride * stem.cin, 1, stem.w, stem.cout, stem.kk * stem.cin, p.net.wdt, w.X + (size_t)b * C, C);
    a.bias = stem.b;
    VV_TRY(vv_linear(&a, stream));
  }
  n = 0;
  items[n++] = vv_rows_item{w.pad0 + stem.cin, p.P0, stem.state, 0, 1, nin, stem.cin, nullptr, nullptr, 0, 0.f, 0.f};          // rows [T, T + ctx), T = 1
  items[n++] = vv_rows_item{w.hpad + ho.cin, p.Kh, ho.state, 0, 1, ho.cin, ho.cin, nullptr, nullptr, 0, 0.f, 0.f};
  VV_TRY(rows_blocks(p, B, w, active, w.hpad + ho.cin, p.Kh, items, &n, s));
  VV_TRY(vv_launch_rows_gemv(VV_ROWS_DEC, B, w.hpad, p.Kh, ho.w, ho.b, nullptr, nullptr, 0, mid, ld_mid, active, s));
  return vv_launch_rows_ctx(items, n, B, p.dl, active, 1, s);
}

extern "C" int vv_encoder_back_rows(const vv_convnet* const* nets, int B, const int* active, const float* mid, int64_t ld_mid, float* feat, int64_t ld_feat,
                                    void* ws, vv_stream_t stream) {
  const char* who = "vv_encoder_back_rows";
  if (!nets || !active || !mid || !feat || !ws) return vv_set_error(VV_E_ARG, "%s: null pointer", who);
  RowsPlan p;
  VV_TRY(rows_plan(who, nets, B, 0, &p));
  const vv_conv& ho = *p.ho;
  const vv_conv& hd = p.net.head;
  const int nmid = ho.stride * ho.cin, nctxh = p.ctxh * ho.cin, nctxd = p.ctxd * hd.cin;
  if (ld_mid < nmid || ld_feat < hd.cout) return vv_set_error(VV_E_ARG, "%s: ld_mid=%lld ld_feat=%lld", who, (long long)ld_mid, (long long)ld_feat);
  hipStream_t s = (hipStream_t)stream;
  RowsWs w;
  rows_carve(p, B, 0, ws, &w);
  vv_rows_item items[VV_ROWS_ITEMS];
  int n = 0;
  items[n++] = vv_rows_item{w.hpad, p.Kh, ho.state, 0, 1, nctxh, ho.cin, nullptr, nullptr, 0, 0.f, 0.f};
  items[n++] = vv_rows_item{w.hpad + nctxh, p.Kh, const_cast<float*>(mid), ld_mid, 0, nmid, ho.cin, nullptr, nullptr, 0, 0.f, 0.f};
  if (nctxd > 0) items[n++] = vv_rows_item{w.hdpad, p.PH, hd.state, 0, 1, nctxd, hd.cin, nullptr, nullptr, 0, 0.f, 0.f};
  VV_TRY(vv_launch_rows_ctx(items, n, B, p.dl, active, 0, s));
  VV_TRY(vv_launch_rows_gemv(VV_ROWS_SEM, B, w.hpad, p.Kh, ho.w, ho.b, nullptr, nullptr, 0, w.X, 2048, nullptr, s));
  n = 0;
  items[n++] = vv_rows_item{w.hpad + nmid, p.Kh, ho.state, 0, 1, nctxh, ho.cin, nullptr, nullptr, 0, 0.f, 0.f};                // rows [T, T + ctx), T = stride
  if (nctxd > 0) items[n++] = vv_rows_item{w.hdpad + hd.cin, p.PH, hd.state, 0, 1, nctxd, hd.cin, nullptr, nullptr, 0, 0.f, 0.f};
  VV_TRY(rows_blocks(p, B, w, active, w.hdpad + nctxd, p.PH, items, &n, s));
  // the head conv (sem_dim outputs, K = kk x 2048): all dialogues' rows in one call, into scratch; the scatter stores the active ones
  vv_lin_args a = lin_base(w.hdpad, p.PH, B, hd.w, hd.cout, hd.kk * hd.cin, p.net.wdt, w.feat, hd.cout);
  a.bias = hd.b;
  VV_TRY(vv_linear(&a, stream));
  items[n++] = vv_rows_item{w.feat, hd.cout, feat, ld_feat, 0, hd.cout, hd.cout, nullptr, nullptr, 0, 0.f, 0.f};
  return vv_launch_rows_ctx(items, n, B, p.dl, active, 1, s);
}

// ---------------------------------------------------------------------------------------------------------------
// SpeechConnector
// ---------------------------------------------------------------------------------------------------------------
extern "C" int vv_connector_forward(const vv_connector* c, const float* x, int R, float* out, int accumulate, float* ws, vv_stream_t stream) {
  if (!c || !x || !out || !ws || R <= 0) return vv_set_error(VV_E_ARG, "vv_connector_forward: bad args");
  vv_lin_args a = lin_base(x, c->din, R, c->fc1, c->hidden, c->din, c->wdt, ws, c->hidden);
  a.bias = c->b1;
  VV_TRY(vv_linear(&a, stream));
  a = lin_base(ws, c->hidden, R, c->fc2, c->hidden, c->hidden, c->wdt, out, c->hidden);
  a.pro = VV_PRO_RMSNORM; a.norm_w = c->norm_w; a.eps = 1e-6f; a.bias = c->b2;
  if (accumulate) { a.res = out; a.ldres = c->hidden; }
  return vv_linear(&a, stream);
}

// acoustic + semantic connector of ONE frame, summed, stored to rows 0 .. rows_out - 1 of out (the next step's input embedding of the positive
// and the negative branch are the same vector, modeling_vibevoice_inference.py:665-673).  ws: 2 * hidden floats.
extern "C" int vv_connector_pair(const vv_connector* ac, const vv_connector* sem, const float* latent, const float* semfeat, float* out, int64_t ldo,
                                 int rows_out, float* ws, vv_stream_t stream) {
  if (!ac || !sem || !latent || !semfeat || !out || !ws || rows_out < 1) return vv_set_error(VV_E_ARG, "vv_connector_pair: bad args");
  const int one = vv_launch_connector_pair(ac, sem, latent, semfeat, out, ldo, rows_out, ws, (hipStream_t)stream);
  if (one) return one < 0 ? one : 0;
  VV_TRY(vv_connector_forward(ac, latent, 1, out, 0, ws, stream));
  VV_TRY(vv_connector_forward(sem, semfeat, 1, out, 1, ws, stream));
  for (int r = 1; r < rows_out; ++r) VV_TRY(vv_copy_rows(out, 0, out + r * ldo, ldo, 1, ac->hidden, stream));
  return 0;
}

// Both connectors for the B dialogues of a row batch: every matrix is read once for all rows; the sums of the ACTIVE dialogues go to rows
// b * rows_out .. + rows_out - 1 of out.  ws: 2 * B * hidden floats
extern "C" int vv_connector_pair_rows(const vv_connector* ac, const vv_connector* sem, const float* latent, int64_t ld_latent, const float* semfeat,
                                      int64_t ld_feat, const int* active, float* out, int64_t ld_out, int rows_out, int B, float* ws, vv_stream_t stream) {
  if (!ac || !sem || !latent || !semfeat || !active || !out || !ws || rows_out < 1) return vv_set_error(VV_E_ARG, "vv_connector_pair_rows: bad args");
  if (B < 2 || B > 8) return vv_set_error(VV_E_UNSUPPORTED, "vv_connector_pair_rows: B=%d (2..8 dialogues)", B);
  if (ac->hidden != sem->hidden || ld_latent < ac->din || ld_feat < sem->din || ld_out < ac->hidden)
    return vv_set_error(VV_E_ARG, "vv_connector_pair_rows: shapes");
  const int H = ac->hidden;
  float* t = ws;
  float* sum = ws + (size_t)B * H;
  const vv_connector* cs[2] = {ac, sem};
  const float* xs[2] = {latent, semfeat};
  const int64_t lds[2] = {ld_latent, ld_feat};
  for (int i = 0; i < 2; ++i) {
    const vv_connector* c = cs[i];
    vv_lin_args a = lin_base(xs[i], lds[i], B, c->fc1, H, c->din, c->wdt, t, H);
    a.bias = c->b1;
    VV_TRY(vv_linear(&a, stream));
    a = lin_base(t, H, B, c->fc2, H, H, c->wdt, sum, H);
    a.pro = VV_PRO_RMSNORM; a.norm_w = c->norm_w; a.eps = 1e-6f; a.bias = c->b2;
    if (i) { a.res = sum; a.ldres = H; }
    VV_TRY(vv_linear(&a, stream));
  }
  return vv_launch_rows_bcast(sum, H, out, ld_out, rows_out, H, B, active, (hipStream_t)stream);
}

extern "C" size_t vv_sizeof(const char* name) {
  if (!name) return 0;
#define S(t) if (!strcmp(name, #t)) return sizeof(t);
  S(vv_w8) S(vv_lin_args) S(vv_kv) S(vv_llm_layer) S(vv_llm) S(vv_head_layer) S(vv_head) S(vv_dpm_coef) S(vv_block) S(vv_conv) S(vv_convnet) S(vv_connector) S(vv_prof_entry) S(vv_nf4_src) S(vv_sampler)
#undef S
  return 0;
}

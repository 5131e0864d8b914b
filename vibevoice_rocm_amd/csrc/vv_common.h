// internal helpers shared by the .hip translation units (not part of the C ABI)
#ifndef VV_COMMON_H
#define VV_COMMON_H
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include "vv_hip.h"

int vv_set_error(int code, const char* fmt, ...);

#define VV_CHECK_LAUNCH(name)                                                                    \
  do {                                                                                           \
    hipError_t e_ = hipGetLastError();                                                           \
    if (e_ != hipSuccess) return vv_set_error(VV_E_HIP, "%s: %s", name, hipGetErrorString(e_));  \
  } while (0)

#define VV_TRY(expr)            \
  do {                          \
    int rc_ = (expr);           \
    if (rc_) return rc_;        \
  } while (0)

// What the attention kernels take by value: vv_kv without the fp8 scale pointers (they travel in vv_kv_args8, to the one kernel that reads
// them), so that growing vv_kv moves no kernel argument of the fp32 / bf16 kernels.
struct vv_kv_args {
  void* k; void* v;
  int kvdt, layers, rows, kv_heads, s_max, head_dim;
  void* vt;
  vv_kv_args(const vv_kv& a) : k(a.k), v(a.v), kvdt(a.kvdt), layers(a.layers), rows(a.rows), kv_heads(a.kv_heads), s_max(a.s_max), head_dim(a.head_dim), vt(a.vt) {}
};
struct vv_kv_args8 : vv_kv_args {
  const float* kscale; const float* vscale;
  vv_kv_args8(const vv_kv& a) : vv_kv_args(a), kscale(a.kscale), vscale(a.vscale) {}
};

// The companions' kind that rides on a descriptor's wdt (VV_WQ_*, vv_hip.h), one line per format: the first bit found wins, no bit = fp8, and vv_wq_strip leaves the matrix dtype in *wdt
// frag_bit / frag_wdt: the bit beside it that says the f_* copies hold the format's fragment-major form, and that form's weight type (0: it has none)
static constexpr struct { int bit, wq, frag_bit, frag_wdt; } VV_WQ_KINDS[] = {
  {VV_WQ_MXFP6, VV_MXFP6, VV_WQ_FRAG6, VV_MXFP6_FRAG},
  {VV_WQ_MXFP4, VV_MXFP4, VV_WQ_FRAG4, VV_MXFP4_FRAG},
  {VV_WQ_NF4, VV_NF4, 0, 0},
};
constexpr int vv_wq_bits() { int bits = VV_WQ_FRAG4 | VV_WQ_FRAG6; for (const auto& k : VV_WQ_KINDS) bits |= k.bit; return bits; }
struct vv_wq_kind { int wq; int fragq; };      // fragq: 0, or the weight type the layers' f_* copies hold - VV_MXFP4_FRAG (VV_WQ_FRAG4) / VV_MXFP6_FRAG (VV_WQ_FRAG6)
static inline vv_wq_kind vv_wq_strip(int* wdt) {
  vv_wq_kind r = {VV_FP8, 0};
  for (const auto& k : VV_WQ_KINDS) if (*wdt & k.bit) { r.wq = k.wq; break; }
  for (const auto& k : VV_WQ_KINDS) if (r.wq == k.wq && k.frag_bit && (*wdt & k.frag_bit)) r.fragq = k.frag_wdt;
  *wdt &= ~vv_wq_bits();
  return r;
}
// The weight-only formats' refusals, one per kernel unit and the only copy of what a call on that unit's formats must be: NULL = taken so far
// (the unit's decision may still find no kernel at this K), else the words for what the call lacks.  Values and alignments only.  *rc (rc may
// be NULL) comes in as VV_E_UNSUPPORTED; a refusal makes it VV_E_ARG where the call is malformed, not merely unserved (fp8 with a bf16 hand-off
// or a shape its fragment-major layout cannot have).  linear_check_args asks them through WQ_FORMATS (vv_kernels.hip), each decision its own.
const char* vv_gemv_stream_refusal(const vv_lin_args& a, int* rc);   // VV_FP8 (row-major), VV_NF4, VV_MXFP4
const char* vv_gemv_mx6_refusal(const vv_lin_args& a, int* rc);      // VV_MXFP6
const char* vv_gemv_rows_refusal(const vv_lin_args& a, int* rc);     // VV_MXFP4_FRAG, VV_FP8 under VV_LIN_W_FRAG
const char* vv_gemv_rows_mx6_refusal(const vv_lin_args& a, int* rc); // VV_MXFP6_FRAG

// The decode GEMV family (m <= 8).  Every launcher is a DECISION - a plain struct computed from the arguments and the vv_tune state, no pointer
// followed, no HIP call, the only copy of the thresholds - and a LAUNCH of that struct; vv_linear_route prints the same struct, so the name it
// reports is the kernel vv_linear starts.  kind 0 = not covered (the caller falls back).
enum { VV_GEMV_STREAM = 1, VV_GEMV_HOT = 2, VV_GEMV_CONV_HOT = 3 };
// vv_gemv_stream.hip: gemv_stream_kernel<m, dual, ksplit, ku, rw, wq> (wq: 0 bf16, 1 fp8, 2 NF4, 3 MXFP4: the VV_MXFP4 weights' streaming GEMV,
// m <= 2, named gemv_mx<m, dual, ksplit, ku>) on blocks x threads, or a hot kernel (table entry idx)
struct vv_stream_route { int kind, idx, m, dual, ksplit, ku, rw, wq, n_groups, blocks, threads; };
vv_stream_route vv_gemv_stream_decide(const vv_lin_args& a);
int vv_launch_gemv_stream_route(const vv_lin_args& a, const vv_stream_route& r, hipStream_t s);   // 1 = launched, 0 = r.kind == 0 or no such kernel
int vv_gemv_stream_route_name(const vv_stream_route& r, char* name, int cap);
// vv_gemv_mx6.hip: gemv_mx6_kernel<m, dual, ksplit, ku>, the VV_MXFP6 weights' streaming GEMV (m <= 2), named gemv_mx6<m, dual, ksplit, ku>
struct vv_mx6_route { int kind, m, dual, ksplit, ku, n_groups, blocks, threads; };
vv_mx6_route vv_gemv_mx6_decide(const vv_lin_args& a);
int vv_launch_gemv_mx6_route(const vv_lin_args& a, const vv_mx6_route& r, hipStream_t s);   // 1 = launched, 0 = r.kind == 0
int vv_gemv_mx6_route_name(const vv_mx6_route& r, char* name, int cap);
void vv_gemv_mx6_set_blocks(int b);                               // tuning hook "gemv_blocks", next to the streaming GEMV's
// vv_gemv_hot.hip: the shape table of the hand-specialised decode GEMVs.  A bf16 vv_linear call whose (m, n, k, dual, prologue kind, epilogue
// kind, flags) equals an entry runs that entry's own kernel when bit i of vv_tune("gemv_hot") is set; every other call takes the generic
// template.  dual: w2 != NULL; mod: adaLN shift / scale rows; bias / gate (per row, gate_ld != 0) / res: that operand is present.
struct vv_gemv_hot_shape { const char* name; int m, n, k, dual, pro, mod, bias, gate, res, act, flags; };
extern "C" int vv_gemv_hot_shapes(vv_gemv_hot_shape* out, int cap);   // copies up to cap entries, returns the table's length (exported for the tests; not in vv_hip.h)
int vv_gemv_hot_covers(const vv_lin_args& a);                     // index of the enabled table entry the call equals, or -1 (no launch)
int vv_launch_gemv_hot(const vv_lin_args& a, int idx, hipStream_t s);   // idx from vv_gemv_hot_covers: 1 = launched on that entry's kernel
void vv_gemv_hot_set(int mask);                                   // tuning hook "gemv_hot"
// vv_conv_hot.hip: the conv tokenizers' one-row stage and hand-over GEMVs on kernels of their own (table: vv_conv_hot_shapes, vv_hip.h); bit i of
// vv_tune("conv_hot") switches entry i.  1 = launched, 0 = no enabled entry matches (the caller goes on to today's path).  The row-batched
// launchers further down start the same kernel templates with 2..8 rows
int vv_conv_hot_gemv_covers(const vv_lin_args& a);                // index of the enabled GEMV table entry the call equals, or -1 (no launch)
int vv_launch_conv_hot_gemv(const vv_lin_args& a, int idx, hipStream_t s);   // idx from vv_conv_hot_gemv_covers: 1 = launched
int vv_launch_conv_hot_row(const vv_block& B, const float* x, float* y, float* hidden, float* hist_new, int C, float eps, hipStream_t s);
void vv_conv_hot_set(int mask);                                   // tuning hook "conv_hot"
// vv_gemv_rows.hip: 3..8 activation rows on the matrix cores, on bf16, fragment-major fp8 or VV_MXFP4_FRAG weights (vv_hip.h), and 9..16 rows on
// fragment-major bf16 weights (gemv_rows16_kernel: two row tiles against every weight load); 1 launched, 0 not
// covered, < 0 error.  part / tickets: split-K workspace (vv_gemv_rows_part_floats / vv_gemv_rows_tickets give the sizes; tickets zero on entry,
// left zero) or null
int vv_launch_gemv_rows(const vv_lin_args& a, float* part, size_t part_floats, int* tickets, size_t n_tickets, hipStream_t s);
// the same, decision apart from launch: gemv_rows_kernel<dual, nw, ks, pers, wf> on (gx, ksplit) blocks, spw weight loads per wave (wf: the weight
// format, 0 = bf16, 1 = fp8, 2 = MXFP4, 3 = MXFP6: 32-, 64-, 128-, 128-wide loads); atomic: the K slices add into out.  have_ws: the caller has a partials workspace
// and tickets (their sizes follow); kind 1 = covered
struct vv_rows_route { int kind, dual, nw, ks, pers, wf, ksplit, spw, atomic, n_groups, gx, rt; };   // rt: row tiles of 8 (2 = gemv_rows16_kernel)
vv_rows_route vv_gemv_rows_decide(const vv_lin_args& a, bool have_ws, size_t part_floats, size_t n_tickets);
int vv_launch_gemv_rows_route(const vv_lin_args& a, const vv_rows_route& r, float* part, int* tickets, hipStream_t s);   // 1 = launched
int vv_gemv_rows_route_name(const vv_rows_route& r, char* name, int cap);
size_t vv_gemv_rows_part_floats(int n, int dual);
size_t vv_gemv_rows_tickets(int n);
int vv_gemv_rows_init();
// vv_gemv_rows_mx6.hip: the same kernel text on VV_MXFP6_FRAG weights, gemv_rows_mx6_kernel<dual, nw, ks, pers> (route wf = 3, named
// gemv_rows_mx6<dual, nw, ks, pers>).  vv_gemv_rows_decide decides and asks which instantiations exist; vv_launch_gemv_rows_route hands over the launch
bool vv_gemv_rows_mx6_built(int dual, int nw, int ks, int pers);
int vv_launch_gemv_rows_mx6_route(const vv_lin_args& a, const vv_rows_route& r, float* part, int* tickets, hipStream_t s);   // 1 = launched
int vv_gemv_rows_mx6_init();                                     // called by vv_gemv_rows_init
void vv_gemv_rows_set(int on, int blocks, int pers);            // tuning hooks (negative / zero: keep)
int vv_linear_ws(const vv_lin_args* a, const void* f1, const void* f2, float* part, size_t part_floats, int* tickets, size_t n_tickets,
                 vv_stream_t stream, const vv_w8* q1 = nullptr, const vv_w8* q2 = nullptr, int fragq = 0);
                 // vv_kernels.hip: f1 / f2 = fragment-major copies of a->w / a->w2 or null; with fp8 companions q1 / q2 (q != NULL) of the fp8 codes;
                 // fragq (VV_WQ_FRAG4 / VV_WQ_FRAG6): f1 / f2 hold the VV_MXFP4_FRAG / VV_MXFP6_FRAG form, codes then scale bytes at byte offset n * k / 2 (n * k * 3 / 4)
int vv_launch_mfma_gemm(const vv_lin_args& a, hipStream_t s);     // vv_mfma_gemm.hip: 1 launched, 0 not covered, <0 error
// the kernel of vv_mfma_gemm.hip a call takes, decided apart from the launch (vv_linear_route reports it without launching): kind 0 = not covered,
// < 0 = error; stream: mfma_linear_kernel<dual, ksplit, xb, mt>, tiled: mfma_tiled_kernel<dual, bk, tm>
enum { VV_MFMA_STREAM = 1, VV_MFMA_TILED = 2 };
struct vv_mfma_route { int kind, dual, ksplit, xb, mt, bk, tm; };
vv_mfma_route vv_mfma_decide(const vv_lin_args& a);
int vv_launch_mfma_route(const vv_lin_args& a, const vv_mfma_route& r, hipStream_t s);   // 1 launched, < 0 error
int vv_mfma_route_name(const vv_mfma_route& r, char* name, int cap);
int vv_mfma_gemm_init();
// vv_gemm_packed.hip: the LDS-DMA 128 x 128 tile GEMM of the packed prompt prefill (gemm_packed_kernel<dual, obf>), taken by VV_LIN_PACKED calls alone.
// vv_gemm_packed_covers is the only copy of what it takes (no launch, no pointer followed); the launch of a covered call returns 0
bool vv_gemm_packed_covers(const vv_lin_args& a);
int vv_launch_gemm_packed(const vv_lin_args& a, hipStream_t s);
int vv_gemm_packed_route_name(const vv_lin_args& a, char* name, int cap);
void vv_gemm_packed_set_rows(int rows);                          // tuning hook "gemm_packed_rows" (0 = never, < 0 = the default)
int vv_gemm_packed_init();
// vv_gemm_mx.hip: the matrix-core GEMM on VV_MXFP4 codes (gemm_mx_kernel<dual, obf>), taken by VV_LIN_W_MXGEMM calls alone.  vv_gemm_mx_check is the
// only copy of what it takes (no launch, no pointer followed): 0, or VV_E_UNSUPPORTED with the reason; the launch of a checked call returns 0
int vv_gemm_mx_check(const vv_lin_args& a);
int vv_launch_gemm_mx(const vv_lin_args& a, hipStream_t s);
int vv_gemm_mx_route_name(const vv_lin_args& a, char* name, int cap);
// vv_gemm_mx6.hip: the same for VV_MXFP6 codes (gemm_mx6_kernel<dual, obf>), taken by VV_LIN_W_MX6GEMM calls alone
int vv_gemm_mx6_check(const vv_lin_args& a);
int vv_launch_gemm_mx6(const vv_lin_args& a, hipStream_t s);
int vv_gemm_mx6_route_name(const vv_lin_args& a, char* name, int cap);
// vv_attn_decode.hip: bf16 KV cache, head_dim 128; part / tickets = split-key workspace ([R, heads, nsplit, 130] floats, [R, heads] zeroed ints) or null
// part_cap: splits the partials workspace has room for (>= nsplit); the grouped kernel may use more splits than the per-head kernel's nsplit
int vv_launch_attn_decode(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const float2* rope, const int* lens, float* out,
                          int64_t ldo, float* part, int* tickets, int nsplit, int part_cap, hipStream_t s);
int vv_attn_decode_ws(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const float* rope_table, const int* lens, float* out,
                      int64_t ldo, float* part, int* tickets, int nsplit, int part_cap, vv_stream_t stream);
int vv_launch_kv_quantize(const vv_kv* src, const vv_kv* dst, int src_row, int dst_row, int len, int flags, hipStream_t s);   // vv_attn_decode.hip
// vv_attn_prefill.hip: matrix-core prompt attention (bf16 cache + kv->vt, head_dim 128).  vv_attn_prefill_covers is the only copy of what the
// kernel covers (vv_attn's route decision asks it, vv_attn_route reports it without a launch); the launch of a covered call: 0 launched, < 0 error
bool vv_attn_prefill_covers(const float* qkv, int64_t ld_qkv, int R, const vv_kv* kv, const float* out, int64_t ldo);
int vv_launch_attn_prefill(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const int* lens, const int* cache_rows,
                           float* out, int64_t ldo, hipStream_t s);
// vv_fused.hip
int vv_head_init_fused(const vv_head* h, const float* noise, float* Xs, float* Ms, float* h0, int64_t ldh, hipStream_t s);
bool vv_head_boundary_supported(const vv_head* h);
int vv_head_boundary_fused(const vv_head* h, const float* hrows, int64_t ldh, const float* shift, const float* scale, int64_t ld_mod, float cfg,
                           const vv_dpm_coef* k, float* Xs, float* Ms, float* h_out, int64_t ldh_out, float* latent_out, hipStream_t s);
int vv_head_boundary_batch(const vv_head* h, const float* hrows, int64_t ldh, const float* shift, const float* scale, int64_t ld_mod, float cfg,
                           const vv_dpm_coef* k, float* Xs, float* Ms, int64_t state_stride, float* h_out, int64_t ldh_out, float* latent_out,
                           int64_t latent_stride, int B, hipStream_t s,   // B dialogues per launch: rows 2 b, 2 b + 1; state / sample of b at b * stride
                           const float* nx = nullptr, int64_t nx_stride = 0,    // SDE: + k->cn * (this step's NX of b at nx + b * nx_stride)
                           const float* cfg_rows = nullptr);                    // device [B]: utterance b's guidance scale, read by its blocks (cfg is not used)
int vv_head_sde_proj_fused(const vv_head* h, const float* sde_noise, int64_t ld_sde, int n_steps, int B, float* NX, hipStream_t s);   // NX[b][i] = [P n ; n], n = sde_noise + b * ld_sde + i * latent
int vv_fused_init();
int vv_head_pre_fused(const vv_head* h, const float* cond2, int64_t ld_cond, const float* temb, int n_steps, void* c_bf16, const float* noise,
                      float* Xs, float* Ms, float* h0, int64_t ldh, hipStream_t s);   // cond_proj + silu(c0 + temb) rows (bf16) + solver-state init in one launch; 1 launched, 0 not covered
int vv_launch_connector_pair(const vv_connector* ac, const vv_connector* sem, const float* latent, const float* semfeat, float* out, int64_t ldo, int rows_out,
                             float* ws, hipStream_t s);   // 1 launched, 0 not covered
int vv_head_modulations_fused(const vv_head* h, const void* c_bf16, int rows, float* const* mod, float* modf, hipStream_t s);   // 1 launched, 0 not covered
// what the three launchers above take, decided once for the launch and for vv_head_sample_route (host only, nothing launched): the kernel's
// template argument (KU of head_pre_kernel / NST of the adaLN kernel: 12 adaln_lds, 28 adaln_all / KU of head_boundary_kernel), 0 = not covered
int vv_head_pre_decide(const vv_head* h, const float* cond2, int64_t ld_cond, const float* temb, int n_steps, const void* c_bf16);
int vv_head_modulations_decide(const vv_head* h, const void* c_bf16, int rows);
int vv_head_boundary_decide(const vv_head* h);
struct vv_conv_ctx_item { float* pad; float* state; int ctx, T, C; const float* dw_w; float* hs; int affine; float scale, bias; };   // dw_w / hs (scatter only): also hs[c] = sum_k<6 dw_w[c, k] * new state[k, c]; affine (gather only): pad = state * scale + bias (the net's input rides along)
int vv_conv_ctx_batch(const vv_conv_ctx_item* items, int n, int scatter, hipStream_t s);   // scatter 0: pad[0:ctx] <- state; 1: state <- pad[T : T + ctx]
// vv_conv_hot.hip, row batches: the one-row stage of the conv tokenizers for the 2..8 dialogues of a row batch in one weight pass.  The dialogues' nets are
// forks of one net: dialogue b's streaming state sits at dialogue 0's address + d[b] floats.  Every launcher: 0 = enqueued, < 0 error
struct vv_rows_delta { int64_t d[8]; };
enum { VV_ROWS_W2 = 0, VV_ROWS_DEC = 1, VV_ROWS_SEM = 2 };       // the three GEMV shapes: block W2 2048 x 8192, hand-overs 8192 x 4096 and 2048 x 16384
int vv_launch_row_in_rows(const vv_block& B, int nb, const float* x, float* y, float* hidden, float* hist_new, const vv_rows_delta& dl, const int* active,
                          float eps, hipStream_t s);             // x / y [nb, 2048], hidden [nb, 8192], hist_new [nb][6, 2048] scratch (active dialogues)
int vv_launch_rows_gemv(int shape, int nb, const float* x, int64_t ldx, const void* w, const float* bias, const float* gate, const float* res,
                        int64_t ldres, float* out, int64_t ldo, const int* active, hipStream_t s);   // active != NULL: only active dialogues' rows are stored
// one move of a gather (buf_b <- other_b [* scale + bias], every dialogue) or a scatter (other_b <- buf_b, active dialogues; with hs also the block
// history's hs_b from the rows stored): buf_b = buf + b * ld_buf, other_b = other + d[b] (relocate: a state pointer of dialogue 0) or + b * ld_other
struct vv_rows_item { float* buf; int64_t ld_buf; float* other; int64_t ld_other; int relocate, n, C; const float* dw_w; float* hs; int affine; float scale, bias; };
#define VV_ROWS_ITEMS 24
int vv_launch_rows_ctx(const vv_rows_item* items, int n, int nb, const vv_rows_delta& dl, const int* active, int scatter, hipStream_t s);
int vv_launch_rows_bcast(const float* src, int64_t ld_src, float* out, int64_t ldo, int rows_out, int n, int nb, const int* active, hipStream_t s);
int vv_block1d_init();                                            // vv_block1d.hip
int vv_launch_block1d(const vv_block& B, int wdt, const float* x, float* out, int T, int C, float eps, hipStream_t s);   // 1 launched, 0 not covered
void vv_block1d_set_fused(int on);
void vv_block1d_set_blocks(int b);
int vv_convffn_init();                                            // vv_convffn.hip
int vv_launch_convffn(const vv_block& B, int wdt, const float* x, float* y, void* hidden, float* hist_new, float* out, int T, int C, float eps,
                      hipStream_t s);                            // 1 launched, 0 not covered
void vv_convffn_set(int on);
int vv_launch_ffn_in_row(const vv_block& B, int wdt, const float* x, float* y, float* hidden, float* hist_new, int C, float eps, hipStream_t s);
void vv_convffn_set_t1(int on);
int vv_launch_ffn_in_row_hs(const vv_block& B, int wdt, const float* x, float* y, float* hidden, float* hist_new, int C, float eps, hipStream_t s);
void vv_convffn_set_t1hs(int on);
void vv_convffn_set_rows(int c, int rows);
void vv_convffn_set_c128(int on);
bool vv_convffn_prefers(int wdt, int T, int C);
int vv_launch_skinny(const vv_lin_args& a, hipStream_t s);       // resampling convs of a streaming frame: 1 launched, 0 not covered
// the decision apart from the launch (vv_linear_route prints it): skinny_kernel<nst, nb>, kind 0 = not covered
struct vv_skinny_route { int kind, nst, nb; };
vv_skinny_route vv_skinny_decide(const vv_lin_args& a);
int vv_skinny_route_name(const vv_skinny_route& r, char* name, int cap);
bool vv_skinny_covers(const vv_lin_args& a);                      // vv_skinny_decide(a).kind != 0
void vv_skinny_set(int on, int min_m, int max_m);
int vv_rmsnorm_rows(const float* x, int64_t ldx, const float* w, float eps, int rows, int n, float* out, int64_t ldo, hipStream_t s,
                    const int* sel = nullptr);                    // sel (device int[rows]) or null: output row r normalises input row sel[r]

#ifdef __HIPCC__
// fp32 -> e4m3fn code, round to nearest even, saturating at +-448 (never the NaN code 0x7f; a NaN input gives +-448): the KV cache's codes
__host__ __device__ __forceinline__ unsigned vv_e4m3_sat(float x) {
  union { float f; unsigned u; } a, t;
  a.f = x;
  const unsigned sign = (a.u >> 24) & 0x80u;
  a.u &= 0x7fffffffu;
  if (!(a.f < 448.f)) a.f = 448.f;
  if (a.u < 0x3c800000u) {             // below 2^-6: subnormal codes, quantum 2^-9 (8 = the smallest normal)
    t.f = a.f * 512.f + 8388608.f;
    return sign | (t.u & 0xffu);
  }
  const unsigned r = (a.u + 0x7ffffu + ((a.u >> 20) & 1u)) >> 20;     // 3 mantissa bits
  return sign | (r - ((127u - 7u) << 3));
}
// GELU (exact-erf form) with erf from Abramowitz & Stegun 7.1.26: |erf error| <= 1.5e-7, one v_exp + one v_rcp + 6 FMA instead
// of libm's erff (~4x the instructions).  The reciprocal is the hardware's v_rcp_f32 (1 ulp): __frcp_rn expands to the IEEE division
// sequence (v_div_scale / v_div_fmas / v_div_fixup + Newton steps, ~10 more instructions per GELU), and these kernels are bound by
// per-CU vector throughput (32 - 64 GELUs per lane per tile: tools/experiments/block1d_x3.hip.inc has the phase timings).  Used only where the result is rounded to bf16 (2^-9 relative) right away - the hidden
// activation between the two FFN GEMMs of a conv block, where every lane evaluates dozens of them and erff was the longest
// phase of the kernel.  fp32 outputs keep erff.
__device__ __forceinline__ float vv_gelu_as(float v) {
  const float x = v * 0.70710678118654752440f, ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
  const float poly = t * fmaf(t, fmaf(t, fmaf(t, fmaf(t, 1.061405429f, -1.453152027f), 1.421413741f), -0.284496736f), 0.254829592f);
  const float erf_abs = 1.0f - poly * __expf(-ax * ax);
  return 0.5f * v * (1.0f + copysignf(erf_abs, x));
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the counter-based generator of the device-side draws:
// the diffusion noise (vv_noise.hip: counter (quad, frame, kind, 0)) and the token draws (vv_token_draw below: counter (quad, position, 0, 1)).
struct philox4 { unsigned x, y, z, w; };

__host__ __device__ __forceinline__ unsigned mulhi32(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

// Philox4x32 with 10 rounds; the key is bumped by the Weyl constants before every round but the first
__host__ __device__ __forceinline__ philox4 philox4x32_10(philox4 c, unsigned k0, unsigned k1) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = mulhi32(M0, c.x), lo0 = M0 * c.x, hi1 = mulhi32(M1, c.z), lo1 = M1 * c.z;
    c = philox4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += W0;
    k1 += W1;
  }
  return c;
}

__device__ __forceinline__ float noise_uniform(unsigned x) { return (float)x * 0x1p-32f + 0x1p-33f; }

// Seeded token draws (vv_hip.h, vv_token_draws): the four exponential draws of quad j (elements 4 j .. 4 j + 3) of the dialogue with `seed` at
// draw index p - the position of the token whose hidden state gives the logits.  Counter (j, p, 0, 1): the fourth word is 1 where the noise
// has 0, so one seed used for both never meets a Philox block twice.  q = -logf(u) with the noise's uniform u in (0, 1]; u == 1 gives 0, which
// becomes the smallest positive normal float: the choice compares p / q.
__device__ __forceinline__ float vv_token_draw_exp(unsigned x) {
  const float q = -logf(noise_uniform(x));
  return q > 0.f ? q : 0x1p-126f;
}
__device__ __forceinline__ float4 vv_token_draw(uint64_t seed, unsigned p, unsigned j) {
  const philox4 x = philox4x32_10(philox4{j, p, 0u, 1u}, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32));
  return make_float4(vv_token_draw_exp(x.x), vv_token_draw_exp(x.y), vv_token_draw_exp(x.z), vv_token_draw_exp(x.w));
}
// q[0 .. nv) of (seed, p), q[nv .. 8) = 1 (vv_sample_choice's masked entries); the second Philox block only when nv reaches it
__device__ __forceinline__ void vv_token_draws8(uint64_t seed, unsigned p, int nv, float (&q)[8]) {
  const float4 a = vv_token_draw(seed, p, 0u);
  float4 b = make_float4(1.f, 1.f, 1.f, 1.f);
  if (nv > 4) b = vv_token_draw(seed, p, 1u);
  const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
  for (int i = 0; i < 8; ++i) q[i] = i < nv ? v[i] : 1.f;
}

// do_sample token choice over nv <= 8 constrained logits (vv_hip.h, vv_sampler: the arithmetic and its order): index of the chosen id.
// One thread; every array index is a compile-time constant after unrolling, so the eight values stay in registers (no scratch): ranks by
// counting instead of a sort - rank_i = #{j : z_j < z_i, or z_j == z_i and j < i} is i's place in the ascending stable sort - and the walk
// over the sorted order as a select per place.  Entries i >= nv ride along as masked ones at the bottom of the order.
__device__ __forceinline__ int vv_sample_choice(const float (&l)[8], int nv, const vv_sampler sp, const float (&q)[8]) {
  constexpr int NV = 8;
  const double ninf = -__builtin_huge_val();
  const double T = (double)sp.temperature;
  double z[NV], e[NV];
  bool keep[NV];
  int rank[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) { keep[i] = i < nv; z[i] = keep[i] ? (double)l[i] / T : ninf; }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    int r = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) r += (j != i && (z[j] < z[i] || (z[j] == z[i] && j < i))) ? 1 : 0;
    rank[i] = r;
  }
  double zmax = ninf;
#pragma unroll
  for (int i = 0; i < NV; ++i) if (rank[i] == NV - 1) zmax = z[i];
  if (sp.top_k > 0 && sp.top_k < nv) {
    double kth = ninf;
#pragma unroll
    for (int i = 0; i < NV; ++i) if (rank[i] == NV - sp.top_k) kth = z[i];
#pragma unroll
    for (int i = 0; i < NV; ++i) keep[i] = keep[i] && !(z[i] < kth);
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) e[i] = keep[i] ? exp(z[i] - zmax) : 0.0;
  if (sp.top_p < 1.f) {
    const double thr = 1.0 - (double)sp.top_p;
    double S = 0.0, cum = 0.0;
#pragma unroll
    for (int r = 0; r < NV; ++r) {
#pragma unroll
      for (int i = 0; i < NV; ++i) if (rank[i] == r) S += e[i];
    }
#pragma unroll
    for (int r = 0; r < NV - 1; ++r) {               // place NV - 1 holds the largest: never removed
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        if (rank[i] == r) {
          cum += e[i] / S;
          if (cum <= thr) keep[i] = false;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) if (!keep[i]) e[i] = 0.0;
  }
  double S = 0.0;
#pragma unroll
  for (int i = 0; i < NV; ++i) S += e[i];
  int best = 0;
  float vbest = (float)(e[0] / S) / q[0];
#pragma unroll
  for (int i = 1; i < NV; ++i) {
    const float v = (float)(e[i] / S) / q[i];
    if (i < nv && v > vbest) { vbest = v; best = i; }
  }
  return best;
}

// Wave-wide (64 lanes) sum, result in every lane.  DPP row operations reduce each 16-lane row at VALU speed (4 dependent
// v_add with a DPP operand), the four row sums are combined through readlane.  The usual __shfl_xor butterfly is six
// dependent ds_bpermute round trips (~100+ cycles each): with one or two waves per SIMD, as in the weight-streaming
// kernels, that latency sits on the critical path of every row group.  Fixed summation order: deterministic.
__device__ __forceinline__ float vv_wave_sum(float v) {
#define VV_DPP_ADD(ctrl) v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xF, 0xF, true))
  VV_DPP_ADD(0xB1);    // quad_perm [1,0,3,2]: lane ^ 1
  VV_DPP_ADD(0x4E);    // quad_perm [2,3,0,1]: lane ^ 2
  VV_DPP_ADD(0x141);   // row_half_mirror: the other quad of the 8-lane half row
  VV_DPP_ADD(0x140);   // row_mirror: the other half of the 16-lane row
#undef VV_DPP_ADD
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
  return (r0 + r1) + (r2 + r3);
}
#endif

#endif

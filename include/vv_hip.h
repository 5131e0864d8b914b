/*
 * vv_hip.h — C ABI of libvv_hip.so: the MI355X (gfx950) kernels of the VibeVoice per-frame hot path.
 *
 * The reference (beecave-homelab/VibeVoice-ROCm) has no native/FFI layer at all: its hot
 * path is Python calling torch ops.  This ABI is therefore the boundary *we* define underneath the reference's
 * Python class API; each entry point names the reference Python code whose arithmetic it replaces
 * (paths relative to the reference root).  The Python host (vibevoice_rocm_amd/) binds it with ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and ints only.  All data pointers are DEVICE pointers unless marked (host).
 *   - every function returns 0 on success, a negative VV_E_* code otherwise; vv_last_error() gives the text
 *     (thread-local).  Nothing throws, nothing allocates device memory: workspaces are caller-provided and sized
 *     with the matching *_ws_bytes() query.  No hidden synchronisation: everything is enqueued on `stream`
 *     and is capturable into a hipGraph (vv_graph_*).
 *   - activations are fp32.  Matrix weights are fp32 or bf16 (`wdt`), vectors (norms, biases, layer scales,
 *     depthwise taps) are always fp32.  KV cache is fp32 or bf16 (`kvdt`), or - decode steps only - e4m3fn bytes with one power-of-two
 *     scale per (layer, KV head) (`kvdt == VV_FP8`, vv_kv.kscale / vscale, filled by vv_kv_quantize).
 *   - convolutional activations are channels-last [T, C] (the reference uses [B, C, T]).
 */
#ifndef VV_HIP_H
#define VV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vv_stream_t; /* hipStream_t */

enum { VV_F32 = 0, VV_BF16 = 1, VV_FP8 = 2 /* e4m3fn bytes + per-output-row fp32 scale (vv_lin_args.wscale); streaming GEMV (m <= 2, row-major) or
                                             3..8-row matrix-core GEMV (VV_LIN_W_FRAG, fp8 fragment-major) only */ };
/* VV_NF4: weight-only 4-bit NF4 (bitsandbytes' blockwise NF4 table, one fp32 absmax per 64 consecutive k of a row), streaming GEMV only:
 * m <= 2, k % 64 == 0, no VV_LIN_W_FRAG.  Effective weight W[n][k] = bf16_rne(table[code] * absmax) (bf16 compute dtype).
 *   w / w2:           packed codes [ceil(N/4)][ceil(K/512)][64 lanes][4 rows][4 B], 16-byte aligned: code of (4 q + r, 512 u + 8 l + i) is
 *                     nibble i (bits 4 i .. 4 i + 3) of dword r of the 16 bytes at ((q * ceil(K/512) + u) * 64 + l) * 16
 *   wscale / w2scale: absmax [ceil(N/4)][ceil(K/512)][4 rows][8 blocks] fp32: block b of unit u covers k = 512 u + 64 b .. + 63
 * Padding (rows past N, k past K) holds code 0 and scale 0.  Any other NF4 call (m > 2, GEMM shapes, VV_LIN_W_FRAG, missing scales) is an error. */
enum { VV_NF4 = 3 };
/* vv_llm.wdt, vv_head.wdt, vv_convnet.wdt: VV_WQ_NF4 ORed into the matrix dtype says the layers' vv_w8 companions hold NF4 (codes in q, block
 * absmax in scale, the VV_NF4 layouts above) instead of fp8.  The 1..2-row GEMVs then stream them; every 3..8-row path (vv_linear_ws,
 * vv_llm_forward with R in 3..8, vv_head_sample_batch(_sde), vv_llm_tail_batch) uses the bf16 matrices (row-major or their bf16 fragment-major
 * f_* copies), which hold the same effective values. */
enum { VV_WQ_NF4 = 0x100 };
/* VV_MXFP4: weight-only OCP Microscaling (MX v1.0) FP4, streaming GEMV only (csrc/vv_gemv_stream.hip, weight format 3): m <= 2, k % 32 == 0, no VV_LIN_W_FRAG, no bf16
 * hand-off.  A block is 32 consecutive k of one row with one E8M0 scale byte e worth 2^(e - 127); elements are e2m1 codes - codes 0..7 mean
 * +0, 0.5, 1, 1.5, 2, 3, 4, 6 and codes 8..15 the same values negated.  Effective weight W[n][k] = value(code) * 2^(e - 127): exact in bf16.
 * Valid scale bytes are 2 <= e <= 252 (every non-zero effective weight is then a normal, finite fp32); the entry points do not read the bytes.
 *   w / w2:           packed codes [ceil(N/4)][ceil(K/512)][64 lanes][4 rows][4 B], 16-byte aligned: code of (4 q + r, 512 u + 8 l + i) is
 *                     nibble i (bits 4 i .. 4 i + 3) of dword r of the 16 bytes at ((q * ceil(K/512) + u) * 64 + l) * 16
 *   wscale / w2scale: the ADDRESS of the scale bytes, read as uint8_t (not as float), 16-byte aligned: [ceil(N/4)][ceil(K/512)][16 blocks][4 rows],
 *                     i.e. the byte of row 4 q + r, block b of unit u (k = 512 u + 32 b .. + 31) at ((q * ceil(K/512) + u) * 16 + b) * 4 + r
 * Padding (rows past N, k past K) holds code 0 and scale byte 127.  Rows of at most 40 units of 512 k (SwiGLU, w2 != NULL: 24).  Any other
 * MXFP4 call (m > 2, k % 32, a missing scale pointer, a misaligned pointer, VV_LIN_W_FRAG, VV_LIN_X_BF16 / VV_LIN_OUT_BF16) returns
 * VV_E_UNSUPPORTED from vv_linear and vv_linear_route alike.  The one other reader of this layout is the matrix-core GEMM on the codes, which a
 * call asks for with VV_LIN_W_MXGEMM (vv_lin_args.flags, below: m >= 3, bf16 x); without that bit nothing above changes. */
enum { VV_MXFP4 = 4 };
/* VV_WQ_MXFP4: as VV_WQ_NF4, for companions that hold MXFP4 (codes in q, the scale bytes' address in scale, the VV_MXFP4 layouts above).  The
 * 1..2-row GEMVs stream them; every 3..8-row path (unless VV_WQ_FRAG4, below) and the prefill use the bf16 matrices, which hold exactly the same
 * effective values - unless the model is LEAN (below, after VV_WQ_FRAG4): its LLM has no bf16 matrices and runs those passes on the codes. */
enum { VV_WQ_MXFP4 = 0x200 };
/* VV_MXFP4_FRAG: the same OCP MXFP4 values (codes, E8M0 scale bytes 2..252, effective weight value(code) * 2^(e - 127)) in FRAGMENT-MAJOR order, for the
 * 3..8-row matrix-core GEMV only (csrc/vv_gemv_rows.hip): VV_LIN_W_FRAG set, 3 <= m <= 8, n % 16 == 0, k % 128 == 0 (no padding occurs), fp32
 * activations and outputs.
 *   w / w2:           codes [N / 16][K / 128][64 lanes][16 B], 16-byte aligned: dword h (0..3) of lane 16 c + n of 128-wide step J of row group g holds
 *                     W[16 g + n][128 J + 32 h + 8 c + i] in nibble i (bits 4 i .. 4 i + 3, the nibble order of VV_MXFP4) - dword h is the B fragment of
 *                     32-wide k step 4 J + h in the lane assignment of the bf16 fragment-major layout; one 1 KB wave load carries four MFMA steps
 *   wscale / w2scale: the ADDRESS of the scale bytes, read as uint8_t, 4-byte aligned: [N / 16][K / 128][16 rows][4 B], i.e. byte h of the dword at
 *                     ((g * K/128 + J) * 16 + n) * 4 is the E8M0 byte of block 4 J + h (k = 128 J + 32 h .. + 31) of row 16 g + n
 * Any other call with this code (m <= 2, m > 8, the flag missing, a missing scale pointer, a misaligned pointer, VV_LIN_X_BF16 / VV_LIN_OUT_BF16,
 * k > 2048 without split-K scratch) returns VV_E_UNSUPPORTED from vv_linear and vv_linear_route alike, the output untouched. */
enum { VV_MXFP4_FRAG = 5 };
/* VV_WQ_FRAG4: ORed into vv_llm.wdt / vv_head.wdt next to VV_WQ_MXFP4 - a layer's f_* pointers then hold the VV_MXFP4_FRAG form of its MXFP4
 * companions: the codes, and the scale bytes behind them in the same allocation at byte offset N * K / 2 (a multiple of 1024).  vv_llm_forward
 * with R in 3..8, vv_linear_ws, vv_head_sample_batch(_sde / _cfg) and the row-batched step around vv_llm_tail_batch then run the MX rows kernel
 * for every matrix that has a copy; a matrix the form cannot take (N % 16, K % 128) keeps f_* = NULL and the bf16 row-major fallback.  The
 * prefill and the m <= 2 calls are unchanged.  No bf16 fragment copy may sit in f_* under this bit. */
enum { VV_WQ_FRAG4 = 0x400 };
/* VV_MXFP6: weight-only OCP Microscaling (MX v1.0) FP6, the e2m3 element type, streaming GEMV only (csrc/vv_gemv_mx6.hip): m <= 2, k % 32 == 0,
 * k <= 24576 (SwiGLU, w2 != NULL: 16384), no VV_LIN_W_FRAG, no bf16 hand-off, no VV_LIN_W_MXGEMM.  A block is 32 consecutive k of one row with
 * one E8M0 scale byte e worth 2^(e - 127); an element is a 6-bit code, sign in bit 5, exponent E in bits 4..3, mantissa m in bits 2..0: E == 0
 * means m / 8, E in 1..3 means (1 + m / 8) * 2^(E - 1), the largest magnitude 7.5.  Effective weight W[n][k] = value(code) * 2^(e - 127): exact
 * in bf16.  Valid scale bytes are 2 <= e <= 252 (every effective weight is then a finite fp32; under e < 5 the smallest elements are fp32
 * subnormals, which the kernel delivers exactly); the entry points do not read the bytes.  With G = ceil(N / 4) row groups and B = K / 32 blocks per row (K is never padded):
 *   w / w2:           codes, 16-byte aligned.  The 32 codes of block b of row 4 q + r form one 192-bit string, code i (k = 32 b + i) in its bits
 *                     6 i .. 6 i + 5 counted from bit 0 of its first byte (little-endian: the operand of v_cvt_scalef32_pk32_f32_fp6 as six
 *                     dwords).  Bytes 0..15 of the string lie in PLANE A of the group, bytes 16..23 in PLANE B: group q occupies the 96 B bytes
 *                     from 96 B q on - plane A [4 rows][B blocks][16 B] in its first 64 B bytes, plane B [4 rows][B blocks][8 B] behind it.
 *                     So a wave that gives lane l block b0 + l of one row reads 1024 contiguous, 16-byte aligned bytes of plane A and 512
 *                     contiguous, 8-byte aligned bytes of plane B.
 *   wscale / w2scale: the ADDRESS of the scale bytes, read as uint8_t (not as float), 4-byte aligned: [G][B blocks][4 rows], i.e. the byte of row
 *                     4 q + r, block b at (q * B + b) * 4 + r - one 4-byte load per lane carries its block's scale in all four rows
 * Padding (rows past N) holds code 0 and scale byte 127.  0.78125 bytes per weight.  Any other MXFP6 call (m > 2, k % 32, a longer row, a missing
 * scale pointer, a misaligned code, scale or activation pointer, VV_LIN_W_FRAG, VV_LIN_X_BF16 / VV_LIN_OUT_BF16, VV_LIN_W_MXGEMM) returns
 * VV_E_UNSUPPORTED from vv_linear and vv_linear_route alike, before any launch, the output untouched.  Value 7 is no weight type.  The 3..8-row
 * matrix-core GEMV reads the same codes in another order, VV_MXFP6_FRAG below: a weight type of its own. */
enum { VV_MXFP6 = 6 };
/* VV_WQ_MXFP6: as VV_WQ_MXFP4, for companions that hold MXFP6 (codes in q, the scale bytes' address in scale, the VV_MXFP6 layout above).  The
 * 1..2-row GEMVs of the LLM, the diffusion head and the tokenizers' one-row stage stream them; every other pass (3 and more rows, the prefill)
 * uses the bf16 matrices, which hold exactly the same effective values - unless VV_WQ_FRAG6 (below) rides along: the 3..8-row decode passes then
 * stream the VV_MXFP6_FRAG copies - and unless the model is LEAN (below, after VV_WQ_FRAG6): its LLM has no bf16 matrices and runs those passes
 * on the codes.  VV_WQ_FRAG4 means nothing next to this bit, and composites that refuse quantised companions refuse these. */
enum { VV_WQ_MXFP6 = 0x800 };
/* VV_MXFP6_FRAG: the same OCP MXFP6 e2m3 values (6-bit codes, E8M0 scale bytes 2..252, effective weight value(code) * 2^(e - 127)) in FRAGMENT-MAJOR
 * order, for the 3..8-row matrix-core GEMV only (csrc/vv_gemv_rows_mx6.hip): VV_LIN_W_FRAG set, 3 <= m <= 8, n % 16 == 0, k % 128 == 0 (no padding
 * occurs), fp32 activations and outputs, no VV_LIN_W_MXGEMM.  gfx950 decodes fp6 32 codes at a time (v_cvt_scalef32_pk32_bf16_fp6), so a LANE OWNS A
 * WHOLE MX BLOCK: lane 16 c + n of 128-wide step J of row group g owns block 4 J + c of row 16 g + n - the 32 codes of k = 128 J + 32 c .. + 31 as
 * the 192-bit string of VV_MXFP6 (code i in bits 6 i .. 6 i + 5, little-endian).  One wave load carries 16 rows x 128 k.
 *   w / w2:           16-byte aligned, (N K 3 / 4 bytes).  Plane A [N / 16][K / 128][64 lanes][16 B]: bytes 0..15 of the lane's string at
 *                     ((g * K/128 + J) * 64 + 16 c + n) * 16.  Plane B [N / 16][K / 128][64 lanes][8 B], at byte offset N * K / 2: bytes 16..23 at
 *                     N K / 2 + ((g * K/128 + J) * 64 + 16 c + n) * 8.  Every wave load is contiguous and naturally aligned (1 KB, 512 B).
 *   wscale / w2scale: the ADDRESS of the scale bytes, read as uint8_t, 4-byte aligned: [N / 16][K / 128][16 rows][4 B] (VV_MXFP4_FRAG's
 *                     arrangement), i.e. byte c of the dword at ((g * K/128 + J) * 16 + n) * 4 is the E8M0 byte of block 4 J + c of row 16 g + n
 * K order: the decoded block is four B fragments - MFMA h (0..3) of the load takes elements 8 h .. 8 h + 7 of every lane's block, the k set
 * {128 J + 32 c + 8 h + i}; the kernel lays the activation fragments out to match.  The summation order is fixed (results repeat bit for bit under
 * vv_tune("gemv_rows_atomic", 0)) but is not the bf16 rows kernel's: against the bf16 fragment-major form of the same effective matrix results
 * agree to fp32 reassociation, never bit for bit.  0.78125 bytes per weight.  Any other call with this code (m <= 2, m > 8, the flag missing, n % 16,
 * k % 128, a missing scale pointer, misaligned codes or scale bytes, VV_LIN_X_BF16 / VV_LIN_OUT_BF16, VV_LIN_W_MXGEMM, k > 2048 without split-K
 * scratch) returns VV_E_UNSUPPORTED from vv_linear and vv_linear_route alike, before any launch, the output untouched. */
enum { VV_MXFP6_FRAG = 8 };
/* VV_WQ_FRAG6: ORed into vv_llm.wdt / vv_head.wdt next to VV_WQ_MXFP6, the counterpart of VV_WQ_FRAG4 - a layer's f_* pointers then hold the
 * VV_MXFP6_FRAG form of its MXFP6 companions: plane A, plane B at byte offset N * K / 2 and the scale bytes at N * K * 3 / 4, one allocation.
 * vv_llm_forward with R in 3..8, vv_linear_ws, vv_head_sample_batch(_sde / _cfg) and the row-batched step around vv_llm_tail_batch then run
 * gemv_rows_mx6_kernel for every matrix that has a copy; a matrix the form cannot take (N % 16, K % 128) keeps f_* = NULL and the bf16 row-major
 * fallback.  1..2 rows and the prefill are unchanged, 9..16 rows stay bf16-only (two passes of 5..8 rows here).  No bf16 fragment copy may sit in
 * f_* under this bit. */
enum { VV_WQ_FRAG6 = 0x1000 };
/* A LEAN MX LLM (vv_llm with VV_WQ_MXFP4 or VV_WQ_MXFP6): every layer's five bf16 pointers (wqkv, wo, wgate, wup, wdown) are NULL beside present
 * companions (q_*.q and q_*.scale) - no descriptor bit, the NULL pointers say it; all five of all layers or none (a mix is VV_E_ARG).  hidden,
 * inter and heads * head_dim must be multiples of 128 and the qkv width a multiple of 16 (what VV_LIN_W_MXGEMM and VV_LIN_W_MX6GEMM take).
 * vv_llm_forward and vv_llm_prefill_packed then run every non-decode pass of R >= 3 rows as the prefill (activations cast to bf16 once per GEMM)
 * on VV_MXFP4 + VV_LIN_W_MXGEMM or VV_MXFP6 + VV_LIN_W_MX6GEMM; R <= 2 streams the companions as ever; a decode pass (cache_rows == NULL) of 3..8
 * rows runs on the VV_MXFP4_FRAG copies under VV_WQ_FRAG4 or the VV_MXFP6_FRAG copies under VV_WQ_FRAG6.  A pass that would need a matrix that is
 * not resident - a 3..8-row decode pass without those copies, a 9..16-row decode pass - returns VV_E_UNSUPPORTED naming the lean mode before
 * anything is launched; no kernel is ever launched on a NULL weight.  vv_llm_ws_bytes counts the bf16 staging buffer from R = 3 on for either
 * lean form. */
enum { VV_OK = 0, VV_E_ARG = -1, VV_E_HIP = -2, VV_E_UNSUPPORTED = -3 };
enum { VV_PRO_NONE = 0, VV_PRO_RMSNORM = 1, VV_PRO_SILU = 2 };
enum { VV_ACT_NONE = 0, VV_ACT_GELU = 1, VV_ACT_SWIGLU = 2 };
/* vv_lin_args.flags: bf16 activation hand-off between two matrix-core GEMMs (x / out point at bf16 [m, ld] arrays, no
 * prologue on a bf16 x), a hint that the weights are re-read soon (keep them cacheable instead of streaming them
 * non-temporally: the diffusion head's matrices are reused by every one of the N solver steps of a frame), and
 * VV_LIN_W_FRAG: w / w2 point at the fragment-major copies of the matrices (vv_llm_layer.f_*; 3..8 rows, n % 16 == 0, bf16 with k % 32 == 0 or
 * fp8 codes with k % 64 == 0 and wscale (w2scale); bf16 copies also at 9..16 rows, the 16-row form of the same GEMV - any other call with this
 * flag is an error).
 * VV_LIN_PACKED: the call belongs to a packed prompt prefill (hundreds to thousands of rows).  With bf16 weights, VV_LIN_X_BF16, no prologue,
 * n % 128 == 0, k % 64 == 0, ldx % 8 == 0, 16-byte aligned operands, an epilogue of bias / residual / VV_ACT_SWIGLU (+ VV_LIN_OUT_BF16) and
 * m >= vv_tune("gemm_packed_rows") (0 = never) it runs on the LDS-DMA tile GEMM of csrc/vv_gemm_packed.hip; any other call routes exactly as
 * without the flag
 * VV_LIN_W_MXGEMM: the matrix-core GEMM on MXFP4 CODES (csrc/vv_gemm_mx.hip) - w / w2 and wscale / w2scale are a VV_MXFP4 companion (wdt ==
 * VV_MXFP4, the layout above, any row and K padding it carries), x is bf16 (VV_LIN_X_BF16, no prologue), m >= 3, n % 16 == 0, k % 128 == 0, the
 * epilogue is bias / residual (its own array or out) / VV_ACT_SWIGLU with w2 (+ VV_LIN_OUT_BF16), no gate.  Codes, scale bytes, x, out, bias and
 * res 16-byte aligned, ldx % 8 == 0, ldo % 4 == 0, ldres % 4 == 0.  The codes are decoded in registers; no bf16 copy of the matrix is read.  No
 * atomics and one fixed K order: a row's result does not depend on the other rows of the call, bit for bit.  Any other call with the bit (another
 * wdt, fp32 x, a prologue, m < 3, n % 16, k % 128, missing scales, a misaligned operand) returns VV_E_UNSUPPORTED from vv_linear and
 * vv_linear_route alike, nothing launched; every VV_MXFP4 / VV_MXFP4_FRAG call without the bit is taken or refused exactly as before */
enum { VV_LIN_X_BF16 = 1, VV_LIN_OUT_BF16 = 2, VV_LIN_W_REUSED = 4, VV_LIN_W_FRAG = 8, VV_LIN_PACKED = 16, VV_LIN_W_MXGEMM = 32 };
/* VV_LIN_W_MX6GEMM: the matrix-core GEMM on MXFP6 CODES (csrc/vv_gemm_mx6.hip), the counterpart of VV_LIN_W_MXGEMM with the same contract - w / w2
 * and wscale / w2scale are a VV_MXFP6 companion (wdt == VV_MXFP6, the two-plane layout above), x is bf16 (VV_LIN_X_BF16, no prologue), m >= 3,
 * n % 16 == 0, k % 128 == 0, the epilogue is bias / residual (its own array or out) / VV_ACT_SWIGLU with w2 (+ VV_LIN_OUT_BF16), no gate.  Codes, x,
 * out, bias and res 16-byte aligned, scale bytes 4-byte aligned, ldx % 8 == 0, ldo % 4 == 0, ldres % 4 == 0.  A lane decodes one whole MX block
 * in registers (v_cvt_scalef32_pk32_bf16_fp6); no bf16 copy of the matrix is read.  No atomics, no split K and one fixed K order (the 128-wide
 * steps ascending, inside a step k = 32 c + 8 h + i with h = 0..3 ascending): a row's result does not depend on the other rows of the call, bit
 * for bit.  The bit is a flag of its own because VV_MXFP6 with VV_LIN_W_MXGEMM is refused, and stays refused.  Any other call with the bit
 * (another wdt, VV_LIN_W_MXGEMM or VV_LIN_W_FRAG beside it, fp32 x, a prologue, m < 3, n % 16, k % 128, missing scales, a gate, a misaligned
 * operand) returns VV_E_UNSUPPORTED from vv_linear and vv_linear_route alike, nothing launched; every call without the bit is taken or refused
 * exactly as before */
enum { VV_LIN_W_MX6GEMM = 64 };

const char* vv_last_error(void);
int vv_abi_version(void);
int vv_tune(const char* key, int value); /* developer tuning hook (grid-size overrides for micro-benchmarks) */
int vv_init(void); /* one-time per-process kernel attribute setup; call before any graph capture */

/* ------------------------------------------------------------------------------------------------------------
 * vv_linear — out[m, n] = epilogue( sum_k W[n, k] * prologue(x)[m, k] )
 * One fused primitive for every Linear / dense Conv1d / ConvTranspose1d of the path:
 *   nn.Linear (q/k/v/o/gate/up/down, heads, connectors, FFN)      x rows contiguous, ldx = k
 *   SConv1d dense, kernel kk, stride s on channels-last data       x = padded [ctx+T, C] buffer, ldx = s*C, k = kk*C
 *   SConvTranspose1d with kk = 2 s                                  x = [1+T, C] buffer, ldx = C, k = 2*C, n = s*C_out
 * prologue (applied to each x row before the product):
 *   VV_PRO_RMSNORM: x * rsqrt(mean(x^2) + eps) [* norm_w] then, if mod_scale != NULL, * (1 + mod_scale[m]) + mod_shift[m]
 *                   (Qwen2RMSNorm; diffusion-head RMSNorm + modulate, modular_vibevoice_diffusion_head.py:31-45;
 *                   ConvRMSNorm, modular_vibevoice_tokenizer.py:77-91; LlamaRMSNorm in SpeechConnector)
 *   VV_PRO_SILU:    silu(x)  (adaLN_modulation / TimestepEmbedder, modular_vibevoice_diffusion_head.py:58-63,152-156)
 * epilogue: + bias[n]; VV_ACT_GELU (erf form, FFN modular_vibevoice_tokenizer.py:589) or VV_ACT_SWIGLU
 *   (silu(W x) * (W2 x), FeedForwardNetwork :116-123 / Qwen2MLP); then * gate (gate_ld == 0: per-channel vector
 *   gate[n] = layer scale gamma; gate_ld > 0: per-row gate[m*gate_ld + n] = adaLN gate); then + res[m*ldres + n].
 * `out` may alias `res`.  m <= 8 rows stream the weights once through a GEMV kernel, larger m use a tiled GEMM.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vv_lin_args {
  const float* x;
  int64_t ldx;
  int m;
  int pro;
  const float* norm_w;
  float eps;
  const float* mod_shift;
  const float* mod_scale;
  int64_t ld_mod;
  const void* w;
  const void* w2;
  const float* bias;
  int n, k, wdt;
  int act;
  const float* gate;
  int64_t gate_ld;
  const float* res;
  int64_t ldres;
  float* out;
  int64_t ldo;
  int flags;   /* VV_LIN_* */
  const float* wscale;   /* wdt == VV_FP8: out = (W8 x) * wscale[n] (+ bias ...); VV_NF4: block absmax; VV_MXFP4 / VV_MXFP4_FRAG / VV_MXFP6 / VV_MXFP6_FRAG: the address of the E8M0 scale bytes, read as uint8_t; else ignored */
  const float* w2scale;
} vv_lin_args;

int vv_linear(const vv_lin_args* a, vv_stream_t stream);
/* The kernel family vv_linear would launch for *a under the current vv_tune state, written to name[cap]: decided by the very code vv_linear
 * launches through, without a launch and without touching the device (pointers count for their alignment only).  For the many-row matrix-core
 * GEMM the instantiation, "mfma_stream<dual=0,ksplit=1,xb=1,mt=4>" or "mfma_tiled<dual=0,bk=128,tm=64>", or "gemm_packed<dual=0,obf=0>" for
 * a VV_LIN_PACKED call its kernel takes (dual: w2 given, obf: VV_LIN_OUT_BF16), "gemm_mx<dual=0,obf=0>" for a VV_LIN_W_MXGEMM call, "gemm_mx6<dual=0,obf=0>" for a VV_LIN_W_MX6GEMM call;
 * "skinny<nst=20,nb=1>" for the resampling convs' skinny GEMM (k = 4 waves x nb bursts x nst steps of 32) and
 * "gemm_f32<w=bf16,dual=0,vec=1,tile=32>" for the fp32 LDS-tiled GEMM (w f32 | bf16; vec: float4 loads; tile 32 | 64); and for the
 * m <= 8 family (fp8, NF4, MXFP4 and MXFP6 weights included) the kernel itself:
 *   "gemv_stream<m=2,dual=0,ksplit=4,ku=3,rw=2,wq=bf16>"                   streaming GEMV (m: 1, 2, 4 or 8 = the template's row count; wq bf16 | fp8 | nf4)
 *   "gemv_mx<m=2,dual=0,ksplit=4,ku=3>"                                    streaming GEMV on VV_MXFP4 weights (m: 1 or 2)
 *   "gemv_mx6<m=2,dual=0,ksplit=5,ku=1>"                                   streaming GEMV on VV_MXFP6 weights (m: 1 or 2; ksplit waves of a block split K, ku units of 2048 k each)
 *   "gemv_rows<dual=0,nw=4,ks=6,pers=0,f8=0> ksplit=5 atomic=0"           3..8-row matrix-core GEMV (taken while vv_tune("gemv_rows_scratch", 1) holds)
 *   "gemv_rows_mx<dual=0,nw=4,ks=3,pers=0> ksplit=6 atomic=0"              the same on VV_MXFP4_FRAG weights (ks: 128-wide weight loads per wave)
 *   "gemv_rows_mx6<dual=0,nw=4,ks=3,pers=0> ksplit=6 atomic=0"             the same on VV_MXFP6_FRAG weights (gemv_rows_mx6_kernel, csrc/vv_gemv_rows_mx6.hip)
 *   "gemv_rows16<dual=0,nw=4,ks=3,pers=0> ksplit=5 atomic=0"               9..16 rows on VV_LIN_W_FRAG bf16 weights: two row tiles per weight load (same condition)
 *   "gemv_hot<3>", "conv_hot_gemv<0>"                                      hot kernels, by table index
 *   "gemv_stream<m=4,...> + gemv_stream<m=2,...>"                          5..8 rows as two streaming passes of 4 + rest rows
 *   "gemv_lds<w=f32,m=3,dual=0,ks=4,np=2>", "gemv_generic<w=bf16>"         the LDS-staged and the generic fall-back
 * Every name fits 128 bytes.  Arguments vv_linear refuses return the same error. */
int vv_linear_route(const vv_lin_args* a, char* name, int cap);

/* ------------------------------------------------------------------------------------------------------------
 * Qwen2 attention pieces (third-party math: transformers.models.qwen2.modeling_qwen2; reference call sites
 * vibevoice/modular/modeling_vibevoice.py:187-199, modeling_vibevoice_inference.py:226-237).
 * KV cache layout: k, v = [layers][rows][kv_heads][s_max][head_dim], dtype kvdt.
 * Each of the R query rows carries lens[r] (device int: its absolute position == number of tokens cached before
 * it) and cache_rows[r] (device int or NULL = r): decode uses rows {positive, negative}; prefill uses R prompt
 * tokens that all append to cache row 0 with lens = pos0 + r.  cache_rows == NULL with R > kv->rows names cache rows the
 * cache does not have: vv_rope_store, vv_attn, vv_llm_forward return VV_E_ARG before anything is launched.
 * vv_rope_store: RoPE (half rotation, fp32 cos/sin from inv_freq) on q and k of qkv[R, (heads+2 kv_heads)*d]
 *   in place, and store k, v at slot lens[r] of the cache.
 * vv_attn: out[r, h*d ..] = softmax(q k^T / sqrt(d)) v over slots 0..lens[r] (inclusive), GQA, fp32 softmax.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vv_kv {
  void* k;
  void* v;
  int kvdt, layers, rows, kv_heads, s_max, head_dim;
  void* vt;   /* optional transposed value cache in 32-key tiles, [layers][rows][kv_heads][s_max / 32][head_dim][32] (same dtype, same size as v):
                 element (d, s) of a head lives at (s / 32) * 32 * head_dim + d * 32 + s % 32, so one tile is 8 KB of contiguous memory whose rows are
                 the A-operand fragments of the matrix-core P.V product.  vv_rope_store and vv_attn_decode keep it in step with v; with it (bf16,
                 head_dim 128, s_max % 32 == 0) prompt-sized vv_attn calls and split-key decode steps run both attention products on the matrix
                 cores without a transpose; NULL: the VALU kernels.  Need not be zero-initialised. */
  /* kvdt == VV_FP8 (head_dim 128, s_max % 32 == 0, s_max >= 64, vt != NULL): k, v and vt keep the layouts above with ONE e4m3fn byte per element, and
     kscale / vscale are fp32 [layers][kv_heads] powers of two shared by all cache rows: the effective value of a code is fp32(code) * scale.
     Only vv_kv_quantize writes such a cache from a prompt and only vv_attn_decode (the grouped-query matrix-core kernel, at every context
     length and key-split count) reads and appends to it; vv_rope_store, vv_attn and the per-head decode kernel return VV_E_UNSUPPORTED.
     kscale / vscale are NULL and ignored for fp32 / bf16 caches. */
  float* kscale;
  float* vscale;
} vv_kv;

/* rope_table[R][head_dim/2][2] = {cos, sin}(lens[r] * inv_freq[i]): computed once per step, shared by all layers */
int vv_rope_table(const int* lens, const float* inv_freq, int R, int head_dim, float* rope_table, vv_stream_t stream);
int vv_rope_store(float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const float* rope_table,
                  const int* lens, const int* cache_rows, vv_stream_t stream);
int vv_attn(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const int* lens,
            const int* cache_rows, float* out, int64_t ldo, vv_stream_t stream);
/* The kernel vv_attn would launch for these arguments under the current vv_tune state, written to name[cap]: decided by the very code vv_attn
 * launches through, without a launch and without touching the device (qkv, out and the cache pointers count for their alignment only):
 *   "attn_prefill_mfma"            both products on the matrix cores (bf16 cache with vt, head_dim 128, R >= 16, s_max % 32 == 0, 16-byte rows)
 *   "attn_group<bf16,nq6,g16>"     one block per (row, KV head), R >= 8, 2 / 6 / 7 q heads per KV head; g = lanes per key when head_dim is 128, else 0
 *   "attn_head<f32>"               one block per (row, q head): everything else
 * Arguments vv_attn refuses return the same error. */
int vv_attn_route(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, const float* out, int64_t ldo, char* name, int cap);
/* vv_attn_decode: vv_rope_store + vv_attn fused for the per-frame step (row r appends to cache row r): qkv is the raw
 * projection (pre-RoPE); q and the new k are rotated in registers, k/v appended at slot lens[r], attention over 0..lens[r]. */
int vv_attn_decode(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const float* rope_table,
                   const int* lens, float* out, int64_t ldo, vv_stream_t stream);
/* The same step with the cached keys of every row split over `nsplit` workgroups per (row, head), as vv_llm_forward runs it on long contexts:
 * part = vv_attn_decode_part_floats(R, heads, part_cap) floats of scratch, tickets = R * heads ints, zero on entry and left zero.  The per-head
 * kernel clamps nsplit to 16 splits of ceil(lens[r] / nsplit) keys.  The grouped kernel launches
 * min(max(min(nsplit, 16), s_max / attn_gqa_keys), part_cap, 64) splits of whole 32-key tiles (vv_tune "attn_gqa_keys": cached keys per split, 1024
 * unless tuned, at least 32), so it may use more than nsplit splits but never more than part_cap >= nsplit nor more than 64: its last workgroup
 * folds at most 16 splits per thread quarter.  Either kernel writes one (m, l, O[128]) record per (row, head, launched split), empty splits
 * included, and nothing else of part.  An fp8 cache (kvdt == VV_FP8) always runs the grouped kernel: the
 * new token's k (after RoPE) and v take part in the step at fp32, and are appended to k, v and vt as codes saturated to +-448 under the head's
 * scale. */
size_t vv_attn_decode_part_floats(int R, int heads, int part_cap);
int vv_attn_decode_split(const float* qkv, int64_t ld_qkv, int R, int heads, const vv_kv* kv, int layer, const float* rope_table,
                         const int* lens, float* out, int64_t ldo, float* part, int* tickets, int nsplit, int part_cap, vv_stream_t stream);
/* vv_kv_quantize - slots [0, len) of row src_row of a bf16 cache (head_dim 128) into row dst_row of an fp8 cache of the same layers / kv_heads
 * (s_max may differ; len <= both): k, v and the tile-major vt of dst, codes = e4m3fn(round-to-nearest-even(clamp(x / scale, -448, 448))) - saturating,
 * never the NaN code.  Slots >= len and every other row are left as they are.  flags & VV_KVQ_DERIVE_SCALES: first sets dst->kscale / vscale of every
 * (layer, KV head) from the absmax of src K / V over those slots, scale = 2^ceil(log2(absmax / 224)) (2x headroom under e4m3's 448; an all-zero
 * head gets 1); without it the scales dst already holds are used.  One launch sequence, no allocation, no synchronisation. */
enum { VV_KVQ_DERIVE_SCALES = 1 };
int vv_kv_quantize(const vv_kv* src_bf16, const vv_kv* dst_fp8, int src_row, int dst_row, int len, int flags, vv_stream_t stream);
/* vv_kv_copy - slots [0, len) of cache row src_row of src -> cache row dst_row of dst, every layer and KV head: k, v, and dst->vt if dst has one.
 * Same kvdt (VV_F32 or VV_BF16), layers, kv_heads, head_dim; rows and s_max may differ (len <= both s_max).  dst->vt is always built from src->v
 * (bf16, head_dim 128, dst s_max % 32 == 0; anything else with dst->vt: VV_E_UNSUPPORTED), so src->vt may be NULL and is never read.  Slots >= len
 * of the destination row (in k, v AND in the last, partial 32-key tile of vt) and every other row are left exactly as they are.  A prefix store -
 * the K / V of a prompt prefix kept for reuse - is an ordinary vv_kv with rows = 1, its own small s_max and vt = NULL: saving a cache row into it
 * and restoring it into a cache are this one call.  src and dst may be the same cache when the rows differ.  VV_FP8 on either side:
 * VV_E_UNSUPPORTED (an fp8 cache is filled through a bf16 staging cache and vv_kv_quantize, as the prompt is).  One launch, no allocation, no
 * synchronisation. */
int vv_kv_copy(const vv_kv* src, int src_row, const vv_kv* dst, int dst_row, int len, vv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Block1D first half on channels-last data (modular_vibevoice_tokenizer.py:924-932 with the streaming
 * SConv1d of :327-382, depthwise k=7):   out = x + gamma * (dwconv7(RMSNorm_c(x)) + b)
 * hist[6, C] holds the previous 6 NORMALISED rows (the conv's cached input) and is updated in place;
 * hist == NULL means non-streaming (zero left context, nothing stored).
 * ------------------------------------------------------------------------------------------------------------ */
int vv_block_mixer(const float* x, float* out, int T, int C, const float* norm_w, float eps, const float* dw_w,
                   const float* dw_b, const float* gamma, float* hist, vv_stream_t stream);
/* The kernel vv_block_mixer would launch for these arguments under the current vv_tune state, written to name[cap]: decided by the very code
 * vv_block_mixer launches through, without a launch and without touching the device (pointers count for NULL, alignment and x == out only):
 *   "mixer_sliced<tr=32,cs=64>"    block_mixer_kernel: workgroups of tr rows x cs channels (cs: power of two <= 64)
 *   "mixer_rows<tr=8,colfix=1>"    mixer_rows_kernel (16 <= T <= 256, C = 256 .. 2048 in steps of 256, vv_tune "mixer_rows"): tr rows x all channels
 *                                  per workgroup; colfix: C / 4 divides 256, the kernel keeps one column's parameters in registers
 * Arguments vv_block_mixer refuses return the same error. */
int vv_block_mixer_route(const float* x, const float* out, int T, int C, const float* norm_w, const float* dw_w, const float* dw_b,
                         const float* gamma, const float* hist, char* name, int cap);

/* Streaming context for the dense convs: pad[0:ctx] <- state; state <- last ctx rows of [state ; pad[ctx:ctx+T]].
 * (SConv1d :364-380 keeps the last ctx inputs; SConvTranspose1d :538-547 needs only the previous input, ctx=1.) */
int vv_conv_ctx(float* pad, float* state, int ctx, int T, int C, vv_stream_t stream);

/* small elementwise helpers */
int vv_affine(const float* x, float a, float b, float* out, int64_t n, vv_stream_t stream);            /* out = a*x + b */
int vv_add_rows(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int rows, int rows_b, int n,
                vv_stream_t stream); /* out[r, :] = a[r / rows_b... see .hip]: c[step*rb + j] = a[j] + b[step]  */
int vv_embed_row(const void* table, int wdt, int64_t hidden, const int* token, float* out, vv_stream_t stream);
int vv_gather_rows(const void* table, int wdt, int64_t hidden, const int* ids_host, int n, void* out, vv_stream_t stream); /* ids (host) */
/* token = ids[argmax logits] (first max in ascending id order, as torch.argmax over the masked vocabulary does,
 * modeling_vibevoice_inference.py:53-66,486-496); *forced_token >= 0 (device int, may be NULL) overrides the choice. */
int vv_argmax_ids(const float* logits, int n, const int* ids, int* token_out, const int* forced_token, vv_stream_t stream);
/* out[r, :] = bf16(prologue(x[r, :])) (prologue: VV_PRO_NONE or VV_PRO_RMSNORM with optional weight): the activation operand of a
 * many-row matrix-core GEMM (vv_linear with VV_LIN_X_BF16), e.g. the prompt prefill */
int vv_cast_rows_bf16(const float* x, int64_t ldx, int rows, int n, int pro, const float* norm_w, float eps, void* out, int64_t ldo,
                      vv_stream_t stream);
int vv_copy_rows(const float* x, int64_t ldx, float* out, int64_t ldo, int rows, int n, vv_stream_t stream); /* ldx may be 0 (broadcast) */
/* one DPM-Solver++ step fused with classifier-free guidance, per latent element
 * (modeling_vibevoice_inference.py:704-707 + vibevoice/schedule/dpm_solver.py:581-584,669-677,738-764):
 *   eps = v_unc + cfg*(v_cond - v_unc); x0 = alpha_s*x - sigma_s*eps;
 *   order 1: x = cx*x - cd*x0;   order 2: x = cx*x - cd*x0 - 0.5*cd*rinv*(x0 - m_prev);   m_prev = x0 */
int vv_dpm_step(const float* v, int64_t ldv, int n_samples, int latent, float cfg_scale, float alpha_s, float sigma_s,
                float cx, float cd, float rinv, int order, float* x, float* m_prev, vv_stream_t stream);
/* positions after a decode step: lens[0] += 1; token == tok_start: lens[1] = 0 (negative branch refreshed, modeling_vibevoice_inference.py:547-563);
 * token == tok_diffusion: lens[1] += 1 (the negative step is committed, :575-587), *frame_counter += 1.  tok_start < 0 selects
 * refresh_negative=False (:501-515): lens[1] += 1 for every token, never reset. */
int vv_advance_lens(int* lens, const int* token, int tok_start, int tok_diffusion, int* frame_counter, vv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Composite operators (one call enqueues the whole launch sequence of a component).
 * ------------------------------------------------------------------------------------------------------------ */
/* Optional weight-only fp8 companion of a matrix for the batch-1/2 decode GEMVs: e4m3fn bytes [N, K] and one
 * fp32 scale per output row.  q == NULL: not quantised.  The bf16 matrix stays the operand of every GEMM-shaped use (prefill, T > 2). */
/* With VV_WQ_NF4 / VV_WQ_MXFP4 / VV_WQ_MXFP6 in the descriptor's wdt the same pair holds an NF4, MXFP4 or MXFP6 companion: q = the packed codes,
 * scale = the block absmax (NF4, fp32) or the address of the E8M0 scale bytes (MXFP4, MXFP6, read as uint8_t), in the VV_NF4 / VV_MXFP4 / VV_MXFP6
 * layouts above. */
typedef struct vv_w8 { const void* q; const float* scale; } vv_w8;

typedef struct vv_llm_layer {
  const float* ln1;  /* input_layernorm.weight */
  const float* ln2;  /* post_attention_layernorm.weight */
  const void* wqkv;  /* rows q | k | v concatenated: [(heads + 2 kv_heads) * d, hidden] */
  const float* bqkv;
  const void* wo;    /* [hidden, heads*d] */
  const void* wgate; /* [inter, hidden] */
  const void* wup;
  const void* wdown; /* [hidden, inter] */
  vv_w8 q_qkv, q_o, q_gate, q_up, q_down;
  /* optional fragment-major copies of the five matrices (NULL: none) for a row-batched decode step (4..8 rows = {positive, negative} x 2..4
   * dialogues; with bf16 copies in every layer also 10..16 rows = 5..8 dialogues; vv_gemv_rows.hip).
   *   bf16 (the matrix has no fp8 companion, q_*.q == NULL): [N / 16][K / 32][4][16][8] bf16, i.e. element (16 g + n, 32 j + 8 c + e) of the
   *   row-major matrix at ((g * K/32 + j) * 64 + 16 c + n) * 8 + e - one matrix-core B fragment per 1 KB of contiguous memory.  N % 16 == 0,
   *   K % 32 == 0.
   *   fp8 (the matrix HAS an fp8 companion, q_*.q != NULL): f_* is then the fragment-major copy of the companion's e4m3fn CODES (its scale is
   *   q_*.scale), [N / 16][K / 64][4][16][2][8] bytes, i.e. code (16 g + n, 64 j + 32 h + 8 c + e) at ((g * K/64 + j) * 64 + 16 c + n) * 16 +
   *   8 h + e - one 1 KB wave load carries the B fragments of two 32-wide k steps.  N % 16 == 0, K % 64 == 0.  Never a bf16 copy.
   *   MXFP4 (VV_WQ_FRAG4 in the descriptor's wdt): f_* is the VV_MXFP4_FRAG form of the MXFP4 companion, codes then scale bytes.  N % 16 == 0,
   *   K % 128 == 0.  Never a bf16 copy.
   *   MXFP6 (VV_WQ_FRAG6 in the descriptor's wdt): f_* is the VV_MXFP6_FRAG form of the MXFP6 companion, plane A, plane B, then scale bytes.
   *   N % 16 == 0, K % 128 == 0.  Never a bf16 copy. */
  const void* f_qkv; const void* f_o; const void* f_gate; const void* f_up; const void* f_down;
} vv_llm_layer;

typedef struct vv_llm {
  int wdt, hidden, inter, layers, heads, kv_heads, head_dim;
  float rms_eps;
  const float* inv_freq;       /* [head_dim/2] */
  const float* final_norm;     /* [hidden] */
  const vv_llm_layer* layer;   /* (host) array [layers] */
} vv_llm;

size_t vv_llm_ws_bytes(const vv_llm* m, int R);
/* R rows of input embeddings x[R, hidden] -> final-normed hidden states out[R, hidden]; appends to the KV cache.
 * Replaces Qwen2Model.forward for both the per-frame decode (R = 2: positive + negative branch sharing one weight
 * pass; modeling_vibevoice_inference.py:478-480 and :581-583) and the prompt prefill (R = L0; :478 at step 0). */
int vv_llm_forward(const vv_llm* m, const vv_kv* kv, const float* x, int64_t ldx, int R, const int* lens,
                   const int* cache_rows, float* out, int64_t ldo, void* ws, vv_stream_t stream);
/* The prompt prefill for the rows of SEVERAL prompts in one weight pass: vv_llm_forward's prefill (R >= 64 rows of a bf16 model; fewer rows run
 * as vv_llm_forward runs them) with VV_LIN_PACKED on its matrix-core linears.  Row r sits at position lens[r] of cache row cache_rows[r]
 * (both device int[R], both required) and reads and writes that (cache row, position) alone: rows of one cache row must be in ascending
 * position order, rows of different cache rows may follow each other in any order.  The final RMSNorm runs on the nsel rows sel[i] only
 * (device int[nsel], each in [0, R)): out is [nsel, hidden].  Workspace: vv_llm_prefill_packed_ws_bytes(m, R).  VV_E_ARG for a null pointer
 * or nsel <= 0, VV_E_UNSUPPORTED for an fp8 cache; no allocation, no synchronisation. */
size_t vv_llm_prefill_packed_ws_bytes(const vv_llm* m, int R);
int vv_llm_prefill_packed(const vv_llm* m, const vv_kv* kv, const float* x, int64_t ldx, int R, const int* lens, const int* cache_rows,
                          const int* sel, int nsel, float* out, int64_t ldo, void* ws, vv_stream_t stream);
/* out == NULL: the final RMSNorm is left to the caller; the un-normalised last hidden rows then stay at the START of ws as [R, hidden] fp32.
 * vv_llm_tail finishes a decode step in one launch: out[R, hidden] = final RMSNorm(h) (the {condition, negative condition} of the
 * diffusion head), logits[nv] = w_valid[nv, hidden] . out[0] (the constrained vocabulary rows of lm_head, VibeVoiceTokenConstraintProcessor
 * modeling_vibevoice_inference.py:53-66), token = ids[argmax] (first maximum in ascending id order) unless *forced_token >= 0, and the
 * position bookkeeping of vv_advance_lens (lens == NULL: skipped). */
int vv_llm_tail(const vv_llm* m, const float* h, int64_t ldh, int R, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion, int* frame_counter,
                vv_stream_t stream);

/* One decode step for B <= 8 dialogues batched into the row dimension: vv_llm_forward with R = 2 B rows (dialogue b = rows 2 b, 2 b + 1 of x, lens and
 * of a KV cache with rows >= 2 B) streams the weights once for all of them; vv_llm_tail_batch then does for every dialogue what vv_llm_tail does
 * for one: h = the un-normalised rows at the start of the LLM workspace, out[2 B, hidden], logits_out[B][8], token_out[B], forced_token[B] or NULL,
 * lens[2 B], frame_counter[B]; active[B] (or NULL = all): a dialogue with active == 0 has finished - its rows are computed and dropped, its
 * positions stay where they are. */
int vv_llm_tail_batch(const vv_llm* m, const float* h, int64_t ldh, int B, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                      float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion, int* frame_counter,
                      const int* active, vv_stream_t stream);

/* do_sample on the device.  The reference draws the token with torch.multinomial(softmax(warped logits), 1) on the host
 * (modeling_vibevoice_inference.py:491-494); on the CPU that is argmax_i(p_i / q_i) with q = empty_like(p).exponential_(1) from the same
 * generator, and the draws q do not depend on the logits - so the host draws q BEFORE it enqueues the step and the device finishes the choice.
 * For nv <= 8 constrained ids, in this order (the HF warpers' order):
 *   1. z_i = double(logit_i) / temperature
 *   2. top-k (0 < top_k < nv): every z_i below the k-th largest becomes -inf
 *   3. top-p (top_p < 1): ascending stable sort, cum = cumsum(softmax(z)) in that order, entries with cum <= 1 - top_p become -inf; the
 *      largest is never removed
 *   4. p_i = float(softmax(z)_i), fp64 up to the cast (a masked id has p = 0)
 *   5. token = ids[argmax_i(p_i / q_i)], the division and the comparison in fp32, first maximum in index order
 * temperature > 0, 0 < top_p <= 1, top_k <= 0: no top-k.  q: nv fp32 values in device memory (exponential draws, > 0). */
typedef struct vv_sampler { float temperature; int top_k; float top_p; } vv_sampler;
/* vv_llm_tail with step 1-5 in place of the argmax.  *forced_token >= 0 still wins (q is then not read for the choice); out, logits_out and
 * the position bookkeeping are those of vv_llm_tail called with the sampled token forced.  VV_E_ARG: temperature <= 0, top_p outside
 * (0, 1], nv > 8, NULL sampler or q. */
int vv_llm_tail_sample(const vv_llm* m, const float* h, int64_t ldh, int R, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                       float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion, int* frame_counter,
                       const vv_sampler* sampler, const float* q, vv_stream_t stream);
/* vv_llm_tail_batch likewise: q[B][8], dialogue b reads q[b][0 .. nv). */
int vv_llm_tail_batch_sample(const vv_llm* m, const float* h, int64_t ldh, int B, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                             float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion,
                             int* frame_counter, const int* active, const vv_sampler* sampler, const float* q, vv_stream_t stream);
/* vv_argmax_ids likewise (the first token after the prompt prefill): logits[n], n <= 8. */
int vv_sample_ids(const float* logits, int n, const int* ids, const vv_sampler* sampler, const float* q, int* token_out, const int* forced_token,
                  vv_stream_t stream);

/* Seeded token draws: per-dialogue warpers and draws that are formed on the device, so that one captured step serves dialogues with different
 * samplers - greedy ones included - and a dialogue's tokens are a function of (its seed, the position, its own logits) alone.
 * The draw q[i], i < nv <= 8, of the dialogue with the 64-bit `seed` at draw index p = the position of the token whose hidden state gives the
 * logits: Philox4x32-10 as in vv_noise_normal with key = (seed & 0xffffffff, seed >> 32) and counter = (i / 4, (uint32) p, 0, 1) - the fourth
 * word is 1 where the noise has 0, so one seed may serve both -, x = output word i % 4, u = (float) x * 2^-32 + 2^-33 in (0, 1], q = -logf(u),
 * and the smallest positive normal float where that is 0 (u == 1).  The choice itself is steps 1-5 above.
 * vv_token_draws: q[b * ldq + i] = the draw of (seeds[b], pos[b * ld_pos] + pos_bias), i < nv; columns nv .. ldq are not written.  seeds, pos
 * are device arrays.  VV_E_ARG, nothing launched: NULL q / seeds / pos, B <= 0, nv outside 1..8, ldq < nv, ld_pos < 0. */
int vv_token_draws(float* q, int64_t ldq, int B, int nv, const uint64_t* seeds, const int* pos, int64_t ld_pos, int pos_bias, vv_stream_t stream);
/* vv_llm_tail_sample / vv_llm_tail_batch_sample with samplers[1] / samplers[B] and seeds[1] / seeds[B] in DEVICE memory in place of the by-value
 * sampler and q: block b reads its own row and seed and forms q from (seeds[b], lens[2 b] as it stands at entry) as vv_token_draws does, bit for
 * bit.  A row with temperature <= 0 is greedy: the argmax of vv_llm_tail (first maximum, smallest id on ties).  *forced_token >= 0 still wins,
 * active == 0 still keeps the positions; out, logits_out, lens and frame_counter are those of vv_llm_tail(_batch) with the chosen token forced.
 * Nothing of the draw is a launch argument: a captured launch serves whatever the arrays hold when it runs.  The caller validates the rows
 * (temperature >= 0, 0 < top_p <= 1); any other row is still memory-safe.  VV_E_ARG, nothing launched: NULL lens / samplers / seeds, nv > 8. */
int vv_llm_tail_sample_rows(const vv_llm* m, const float* h, int64_t ldh, int R, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                            float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion, int* frame_counter,
                            const vv_sampler* samplers, const uint64_t* seeds, vv_stream_t stream);
int vv_llm_tail_batch_sample_rows(const vv_llm* m, const float* h, int64_t ldh, int B, float* out, int64_t ldo, const void* w_valid, int nv, const int* ids,
                                  float* logits_out, int* token_out, const int* forced_token, int* lens, int tok_start, int tok_diffusion,
                                  int* frame_counter, const int* active, const vv_sampler* samplers, const uint64_t* seeds, vv_stream_t stream);

typedef struct vv_head_layer {
  const float* norm_w;
  const void* wgate;  /* [ffn, D] */
  const void* wup;
  const void* wdown;  /* [D, ffn] */
  const void* adaln;  /* [3D, D]: shift | scale | gate */
  vv_w8 q_gate, q_up, q_down;
  const void* f_gate; const void* f_up; const void* f_down;   /* optional fragment-major copies, bf16 or - with q_*.q set - fp8 codes (see vv_llm_layer) */
} vv_head_layer;

typedef struct vv_head {
  int wdt, D, ffn, layers, latent, cond_dim;
  float eps;
  int flags;                 /* reserved, 0 */
  const void* noisy_proj;    /* [D, latent] */
  const void* cond_proj;     /* [D, cond_dim] */
  const void* final_adaln;   /* [2D, D]: shift | scale */
  const void* final_linear;  /* [latent, D] */
  const vv_head_layer* layer; /* (host) array */
  const float* fused_g;      /* optional [D + latent, D] fp32: [noisy_proj x final_linear ; final_linear].  When set, vv_head_sample runs a solver-step
                                boundary (FinalLayer + CFG + DPM-Solver++ update + next noisy_images_proj: all linear in the modulated hidden state) as
                                ONE GEMV over it with the solver as epilogue; NULL keeps the three-launch form */
} vv_head;

typedef struct vv_dpm_coef { float alpha_s, sigma_s, cx, cd, rinv; int order; float cn; /* variance-noise coefficient: 0 for the ODE solver, sigma_t sqrt(1 - e^-2h) for sde-dpmsolver++ */ } vv_dpm_coef;

/* out[(i*rows_b + j), :] = silu(a[j, :] + b[i, :]): the adaLN input silu(cond_proj(cond) + t_emb(t_i)) for all steps at once */
int vv_add_rows_silu(const float* a, int64_t lda, const float* b, int64_t ldb, float* out, int rows, int rows_b, int n, vv_stream_t stream);
/* same, rounded to bf16 [rows, n] (the VV_LIN_X_BF16 operand of the hoisted adaLN GEMMs) */
int vv_add_rows_silu_bf16(const float* a, int64_t lda, const float* b, int64_t ldb, void* out, int rows, int rows_b, int n, vv_stream_t stream);
/* step boundary of the sampler in one launch: x_out = DPM-Solver++/CFG update of (v, x_in, m_in) [v == NULL: x_out = x_in],
 * m_out = x0 prediction, and h[r, :] = W x_out for r < rows (the next step's noisy_images_proj; W == NULL: skipped).
 * x_in/x_out and m_in/m_out must be distinct buffers. */
int vv_dpm_proj(const float* v, int64_t ldv, float cfg_scale, const vv_dpm_coef* coef, const float* x_in, const float* m_in,
                float* x_out, float* m_out, const void* w, int wdt, int latent, int D, float* h, int64_t ldh, int rows,
                const float* step_noise /* [latent] variance noise of this step (coef->cn != 0) or NULL */, vv_stream_t stream);

size_t vv_head_ws_bytes(const vv_head* h, int n_steps);
/* sample_speech_tokens for ONE utterance (modeling_vibevoice_inference.py:695-708) with
 * VibeVoiceDiffusionHead.forward (modular_vibevoice_diffusion_head.py:254-280) and the DPM-Solver++ step
 * (vibevoice/schedule/dpm_solver.py:935-1022) fused into one launch sequence:
 *   cond2[2, cond_dim] = {positive, negative} LLM hidden states; noise[latent]; temb[n_steps, D] = t_embedder(t_i)
 *   (step-invariant, precomputed by the host with vv_linear); coef (host) per step.  latent_out[latent].
 * cond_proj and every adaLN modulation are hoisted out of the step loop (they do not depend on x). */
int vv_head_sample(const vv_head* h, const float* cond2, int64_t ld_cond, const float* noise, const float* temb,
                   const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, void* ws,
                   const float* sde_noise /* [n_steps, latent] per-step variance noise of the SDE solver (dpm_solver.py:993-998) or NULL */,
                   vv_stream_t stream);
/* sample_speech_tokens for B utterances at once (B <= 8; 5..8 - 10..16 rows - on the bf16 matrices and their bf16 fragment-major copies alone; the ODE solver on the fused boundary - SDE coefficients return VV_E_UNSUPPORTED; bf16 weights, with
 * their fp8 companions' fragment-major codes where the layers carry them, or - VV_WQ_FRAG4 - the VV_MXFP4_FRAG form of their MXFP4 companions): cond[2 B, cond_dim] = rows
 * {positive, negative} of utterance b at 2 b, 2 b + 1; noise[b * ld_noise ..], latent_out[b * ld_latent ..].  Every head matrix is streamed once
 * per solver step for all utterances.  ws: vv_head_ws_bytes_batch(h, n_steps, B) bytes. */
size_t vv_head_ws_bytes_batch(const vv_head* h, int n_steps, int B);
int vv_head_sample_batch(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                         const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, int64_t ld_latent, int B, void* ws,
                         vv_stream_t stream);
/* The same with the SDE solver (sde-dpmsolver++, coef[i].cn != 0): sde_noise[B][n_steps][latent] (utterance b at b * ld_sde, step i at
 * i * latent) is the per-step variance noise, step i of utterance b adding coef[i].cn * sde_noise[b][i] to x - the row vv_head_sample takes
 * at sde_noise + i * latent, so both give the same sample.  One launch before the step loop maps all of it into the solver state
 * ([noisy_proj n ; n]); the fused boundary adds it in its epilogue.  sde_noise == NULL: the ODE solver, bit-identical to vv_head_sample_batch.
 * ws: vv_head_ws_bytes_batch_sde(h, n_steps, B) bytes. */
size_t vv_head_ws_bytes_batch_sde(const vv_head* h, int n_steps, int B);
int vv_head_sample_batch_sde(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                             const vv_dpm_coef* coef, int n_steps, float cfg_scale, float* latent_out, int64_t ld_latent, int B, void* ws,
                             const float* sde_noise, int64_t ld_sde, vv_stream_t stream);
/* The same two samplers with one guidance scale PER UTTERANCE, read on the device: cfg_rows[B] (device memory; utterance b's scale) takes the
 * place of cfg_scale, so a captured graph serves any scales and utterances with different scales share a call.  sde_noise == NULL: the ODE
 * solver with the workspace of vv_head_ws_bytes_batch; else the SDE solver with that of vv_head_ws_bytes_batch_sde.  Same limits and argument
 * errors as those; cfg_rows == NULL returns VV_E_ARG.  With cfg_rows[b] == c for all b the sample is that of the scalar entry point at c. */
int vv_head_sample_batch_cfg(const vv_head* h, const float* cond, int64_t ld_cond, const float* noise, int64_t ld_noise, const float* temb,
                             const vv_dpm_coef* coef, int n_steps, const float* cfg_rows /* device, [B] */, float* latent_out, int64_t ld_latent,
                             int B, void* ws, const float* sde_noise /* NULL: ODE */, int64_t ld_sde, vv_stream_t stream);
/* vv_head_sample_route - the stage kernels a sampler call with these arguments takes, by the decisions the call itself makes (one copy of each
 * condition, shared with the launch path); nothing is launched and no device pointer is followed (pointers count for NULL and alignment; coef,
 * a host array, is read for coef[i].cn).  B = 0: vv_head_sample(h, cond, ld_cond, .., temb, coef, n_steps, .., ws, sde ? noise : NULL).
 * B >= 1: the batched entry points - cfg_rows != NULL vv_head_sample_batch_cfg, else sde != 0 vv_head_sample_batch_sde, else
 * vv_head_sample_batch; sde != 0 stands for a non-NULL sde_noise with a sufficient ld_sde.  noise and latent_out are taken as given.
 * name (cap bytes) becomes "pre=<..> mod=<..> step=<..>":
 *   pre   "head_pre<ku=K>"                         head_pre_kernel<K> (cond_dim = 512 K): cond_proj, the bf16 conditioning rows and the solver state
 *         "linear+add_rows_silu_bf16+head_init<bf16>"   vv_linear, vv_add_rows_silu_bf16, head_init_kernel<bf16_t>: the batched samplers always, the
 *                                                  single one where head_pre does not cover the call (cond_dim % 512, n_steps > 128, latent > 256, ..)
 *         "linear+add_rows_silu+head_init<bf16|f32>"    fp32 conditioning rows (n_steps <= 4, D % 32, fp32 weights) in front of the fused boundary
 *         "linear+add_rows_silu[_bf16]"            the same in front of the three-launch step (vv_dpm_proj initialises the state)
 *         "...+head_sde_proj<bf16>"                batched with variance noise: head_sde_proj_kernel maps it into state space before the loop
 *   mod   "adaln_lds<nst=12>" (D = 1536), "adaln_all<nst=28,nm=1>" (D = 3584): every adaLN matrix in one launch; "linear": one vv_linear each
 *   step  "boundary<ku=K,sde=S,cfg=C>"             head_boundary_kernel<K, S> (C = 1: head_boundary_cfg_kernel<K, S>), K = ceil(D / 512); S = 1: the
 *                                                  steps with coef[i].cn != 0 run the SDE instantiation, the others (and every step at S = 0) <K, false>
 *         "dpm_proj"                               vv_dpm_proj + the FinalLayer vv_linear: fused_g NULL / unaligned, D % 8, D > 4096, or vv_head_sample
 *                                                  with variance noise or a coef[i].cn != 0
 * Arguments the sampler refuses return the sampler's error (VV_E_ARG / VV_E_UNSUPPORTED, vv_last_error names the entry point); VV_E_ARG also for
 * name == NULL, cap <= 0, B < 0 and cfg_rows with B = 0. */
int vv_head_sample_route(const vv_head* h, const float* cond, int64_t ld_cond, const float* temb, const vv_dpm_coef* coef, int n_steps, int B,
                         int sde, const float* cfg_rows, const void* ws, char* name, int cap);
/* vv_head_ws_layout - byte offsets of the regions the samplers carve out of ws, from the carving code they run (B = 0: vv_head_sample; B >= 1
 * the batched samplers, sde != 0: with variance noise).  off[] in this order, -1 = the form has no such region; returns the number of entries
 * written (layers + 10, + 5 for B = 0) or an error (VV_E_ARG: NULL h / off, n_steps <= 0, layers > 16, B outside 0..8, sde with B = 0, cap too small):
 *   c0      fp32 [2 | 2 B rows, D] cond_proj output (not written where head_pre runs)
 *   c       conditioning rows silu(c0 + temb_i), row (i * 2 B + r); bf16 [rows, D] packed, or fp32 [rows, D] where the route's pre says add_rows_silu
 *   mod[l]  l < layers: fp32 [rows, 3 D] shift | scale | gate of layer l        modf    fp32 [rows, 2 D] shift | scale of the FinalLayer
 *   h0, h1  the two hidden-row buffers [2 | 2 B rows, D]: step i's layers work in h(i & 1), its boundary writes h((i + 1) & 1)
 *   act     [rows, ffn]        Xs, Ms   solver state [P x ; x] and previous x0 prediction, utterance b at b * (D + latent) floats
 *   NX      SDE, batched: [B][n_steps][D + latent] variance noise in state space, else -1
 *   B = 0 only - the three-launch form's v [2, latent], x double buffer (2 entries), x0-history double buffer (2 entries)
 *   end     bytes carved = vv_head_ws_bytes / vv_head_ws_bytes_batch(_sde) */
int vv_head_ws_layout(const vv_head* h, int n_steps, int B, int sde, int64_t* off, int cap);
/* The samplers' Gaussian noise drawn on the device, one launch for B utterances: noise[b * ld_noise + e], e < n, is the initial latent (kind 0) and,
 * when sde_noise is given, sde_noise[b * ld_sde + s * n + e] the variance noise of solver step s < n_steps (kind 1 + s) - the buffers
 * vv_head_sample and vv_head_sample_batch(_sde) read.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85)
 * with key = (seeds[b] & 0xffffffff, seeds[b] >> 32) and counter = (j, (uint32) frames[b], kind, 0) gives the four values of quad j (elements
 * 4 j .. 4 j + 3): u_i = (float) x_i * 2^-32 + 2^-33 in (0, 1], z[4 j] = r(u0) cos(2 pi u1), z[4 j + 1] = r(u0) sin(2 pi u1), z[4 j + 2] and
 * z[4 j + 3] likewise from (u2, u3), r(u) = sqrtf(-2 logf(u)); elements >= n of the last quad are dropped, columns n .. ld are not written.  A
 * row is a function of (seed, frame, kind) alone: not of B, of the row's place in the call or of anything drawn before.  seeds and frames
 * are device arrays [B], every other argument a pointer or a shape: the launch can be captured into a graph.  VV_E_ARG, nothing launched:
 * NULL noise / seeds / frames, B <= 0, n <= 0, n_steps < 0, ld_noise < n, ld_sde < n_steps * n with sde_noise given. */
int vv_noise_normal(float* noise, int64_t ld_noise, float* sde_noise, int64_t ld_sde, int B, int n, int n_steps, const uint64_t* seeds,
                    const int* frames, vv_stream_t stream);
/* VibeVoiceDiffusionHead.forward alone (parity tests): x[R, latent], temb_rows[R, D], cond[R, cond_dim] -> v[R, latent] */
int vv_head_forward(const vv_head* h, const float* x, const float* temb_rows, const float* cond, int R, float* v,
                    void* ws, vv_stream_t stream);

typedef struct vv_block {
  const float* gamma; const float* ffn_gamma; const float* norm_w; const float* ffn_norm_w;
  const float* dw_w;  /* [C, 7] */
  const float* dw_b;
  const void* w1; const float* b1;  /* [4C, C] */
  const void* w2; const float* b2;  /* [C, 4C] */
  float* hist;                      /* [6, C] streaming state or NULL */
  vv_w8 q_w1, q_w2;                 /* used when the block runs as GEMVs (T <= 2 rows: stage 0 of a streaming frame) */
  const float* dw_last;             /* optional [C]: dw_w[:, 6] packed (the tap of the newest row); with hs: one-row frames skip the 7-row window */
  float* hs;                        /* optional [C] streaming state next to hist: sum_k<6 dw_w[c, k] * hist[k, c], kept in step with hist by
                                       the composites (zero when hist is zero); NULL = recompute from hist every frame */
} vv_block;

/* One whole Block1D (mixer + FFN, vibevoice/modular/modular_vibevoice_tokenizer.py:555-600) as a single launch: x[T, C] -> out[T, C]
 * (out != x).  Covered: bf16 weights, C = 32 / 64 / 128, T >= 32; anything else returns VV_E_UNSUPPORTED (the composites then
 * run vv_block_mixer + two vv_linear).  b->hist (or NULL) is the streaming state, updated in place. */
int vv_block1d(const struct vv_block* b, int wdt, const float* x, float* out, int T, int C, float eps, vv_stream_t stream);
/* The kernel vv_block1d would launch, as vv_block_mixer_route: "block1d<c=128> grid=3" - grid workgroups of 32-row tiles; grid below
 * ceil(T / 32) (C = 128 above vv_tune "block1d_blocks" tiles) is the persistent walk, workgroup g taking tiles g, g + grid, ...  Pointers (x, out,
 * the block's arrays) count for NULL, alignment and overlap only.  Arguments vv_block1d refuses return the same error. */
int vv_block1d_route(const struct vv_block* b, int wdt, const float* x, const float* out, int T, int C, char* name, int cap);

/* The same Block1D for the middle stages of a streaming frame (bf16 weights; C = 256 / 512 with 3 <= T <= 256, C = 1024 with T <= 64,
 * C = 128 with T <= 1024) as two launches (mixer +
 * first FFN GEMM, second FFN GEMM): x[T, C] -> out[T, C] (out != x).  ws: vv_block_mid_ws_bytes(T, C) bytes of scratch, 16-byte aligned.
 * Other shapes return VV_E_UNSUPPORTED.  b->hist as above.
 * After the call ws holds, from its start: y = the mixer output (the FFN's residual) as [T, C] fp32, then the hidden activation
 * gelu(W1 RMSNorm(y) + b1) as [T, 4C] bf16; the rest (6 * C floats + padding) is scratch for the history hand-over.  out may be the start of ws
 * (out == y: the second launch then adds the FFN branch to y in place - the form the convnet composites use for every middle block); any other
 * overlap of out with ws, or of x with the first T * C floats of ws, is not allowed. */
size_t vv_block_mid_ws_bytes(int T, int C);
int vv_block_mid(const struct vv_block* b, int wdt, const float* x, float* out, void* ws, int T, int C, float eps, vv_stream_t stream);
/* The two kernels vv_block_mid would launch, as vv_block_mixer_route: "ffn_in<c=512,trv=8,nt=512> + ffn_out<c=512,nw=4>" - trv: rows per
 * workgroup of the first launch (vv_tune "convffn_rows512" / "convffn_rows256" / "convffn_rows128": 8 | 16 | 32, 16 | 32 at C = 128; C = 1024
 * always 8), nt its threads, nw the waves that split K in the second.  Pointers count for NULL, alignment and overlap only.  Arguments
 * vv_block_mid refuses return the same error. */
int vv_block_mid_route(const struct vv_block* b, int wdt, const float* x, const float* out, const void* ws, int T, int C, char* name, int cap);

typedef struct vv_conv {
  const void* w;      /* re-laid: SConv1d [cout, kk*cin] with k index = tap*cin + ci;
                         SConvTranspose1d [s*cout, 2*cin] with row = r*cout + co, k = j*cin + ci (j=0: previous input) */
  const float* b;     /* SConv1d [cout];  SConvTranspose1d [s*cout] (bias tiled over r) */
  int cin, cout, kk, stride, transposed;
  float* state;       /* [ctx, cin] streaming state or NULL; ctx = kk - stride (conv) or 1 (transposed) */
} vv_conv;

#define VV_MAX_STAGES 8
typedef struct vv_convnet {
  int wdt, n_stages;
  float eps;
  vv_conv sample[VV_MAX_STAGES];          /* stem + up/down-sampling convs, one per stage */
  int n_blocks[VV_MAX_STAGES];
  const vv_block* blocks[VV_MAX_STAGES];  /* (host) arrays */
  vv_conv head;
} vv_convnet;

size_t vv_convnet_ws_bytes(const vv_convnet* net, int64_t t_in, int decoder);
/* TokenizerDecoder.forward (modular_vibevoice_tokenizer.py:914-951): latent[T, vae_dim] -> wav[T*hop] (streaming
 * when the net carries state buffers).  pre_scale/pre_bias fold `latent / scale - bias`
 * (modeling_vibevoice_inference.py:634) into the stem input: x = pre_scale*latent + pre_bias. */
int vv_decoder_forward(const vv_convnet* net, const float* latent, int T, float pre_scale, float pre_bias, float* wav,
                       void* ws, vv_stream_t stream);
/* TokenizerEncoder.forward (:776-813): wav[T] -> feat[ceil(T/hop), vae_dim]; streaming (T multiple of hop, net has
 * state) or whole-utterance non-streaming with the reference's zero left/right padding (:384-418). */
int vv_encoder_forward(const vv_convnet* net, const float* wav, int64_t T, float* feat, void* ws, vv_stream_t stream);
/* zero every state buffer of the net == VibeVoiceTokenizerStreamingCache.set_to_zero (:234-241) */
int vv_convnet_reset(const vv_convnet* net, vv_stream_t stream);

typedef struct vv_connector { int wdt, din, hidden; const void* fc1; const float* b1; const float* norm_w; const void* fc2; const float* b2; } vv_connector;
/* SpeechConnector.forward (modeling_vibevoice.py:58-69): out[R,hidden] (+)= fc2(RMSNorm(fc1 x)); accumulate != 0 adds
 * into `out` (acoustic + semantic sum, modeling_vibevoice_inference.py:665-667).  ws: R*hidden floats. */
int vv_connector_forward(const vv_connector* c, const float* x, int R, float* out, int accumulate, float* ws, vv_stream_t stream);
/* Both connectors of one generated frame: out[r, :] = acoustic_connector(latent) + semantic_connector(semfeat) for r < rows_out
 * (modeling_vibevoice_inference.py:665-670; the positive and the negative branch consume the same embedding, :575-579).  Two launches
 * (fc1 of both, fc2 of both with the RMSNorms in the prologue) when the weights are bf16, else the two connectors in turn.  ws: 2 * hidden floats. */
int vv_connector_pair(const vv_connector* ac, const vv_connector* sem, const float* latent, const float* semfeat, float* out, int64_t ldo,
                      int rows_out, float* ws, vv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row-batched conv tails: the one-row stage (C = 2048, one row per frame) of both streaming tokenizers for the B dialogues of a row batch in
 * ONE pass over its weights (csrc/vv_conv_hot.hip), every dialogue on its own streaming state.
 *   nets:    (host) array of B nets that are forks of one net - the same weight pointers, every state pointer moved by one offset per dialogue
 *            (DeviceWeights.fork) - anything else is VV_E_ARG
 *   active:  device int[B]; a dialogue with active == 0 rides along: its rows are computed from whatever the buffers hold and dropped - no
 *            store reaches its state or its output row
 * Covered: bf16 weights without companions, a streaming net whose one-row stage is C = 2048 with hs / dw_last on every block, 2 <= B <= 8;
 * anything else is VV_E_UNSUPPORTED, bad arguments VV_E_ARG, both before any launch.  No allocation, no synchronisation, capturable.
 *   vv_decoder_front_rows     context gather, stem conv, the one-row blocks, the transposed hand-over conv 2048 -> 8 x 1024: row b of mid
 *                             (pitch ld_mid >= 8192) = dialogue b's input of the C = 1024 stage; latent row b at latent + b * ld_latent
 *   vv_decoder_forward_from   the remaining stages and the head conv of ONE dialogue and one frame from its mid row, with their state: wav.
 *                             vv_decoder_front_rows then vv_decoder_forward_from leave dialogue b's state and waveform as vv_decoder_forward does
 *   vv_encoder_forward_until  ONE dialogue: stem up to and including the C = 1024 stage; mid = its [T / hop x 8, 1024] rows
 *   vv_encoder_back_rows      each dialogue's hand-over conv context, the hand-over conv 16 x 1024 -> 2048, the one-row blocks, the head conv:
 *                             feat[b * ld_feat ..] = dialogue b's feature.  vv_encoder_forward_until then vv_encoder_back_rows = vv_encoder_forward
 *   vv_connector_pair_rows    vv_connector_pair for B dialogues: out rows b * rows_out .. + rows_out - 1 (pitch ld_out) for the active ones;
 *                             ws: 2 * B * hidden floats
 * Workspaces: vv_conv_rows_ws_bytes(net, B, decoder) for the two *_rows composites (0: not covered), vv_convnet_ws_bytes(net, T, decoder) for
 * vv_decoder_forward_from (T = 1) and vv_encoder_forward_until.
 * ------------------------------------------------------------------------------------------------------------ */
size_t vv_conv_rows_ws_bytes(const vv_convnet* net, int B, int decoder);
int vv_decoder_front_rows(const vv_convnet* const* nets, int B, const int* active, const float* latent, int64_t ld_latent,
                          float pre_scale, float pre_bias, float* mid, int64_t ld_mid, void* ws, vv_stream_t stream);
int vv_decoder_forward_from(const vv_convnet* net, const float* mid, float* wav, void* ws, vv_stream_t stream);
int vv_encoder_forward_until(const vv_convnet* net, const float* wav, int64_t T, float* mid, void* ws, vv_stream_t stream);
int vv_encoder_back_rows(const vv_convnet* const* nets, int B, const int* active, const float* mid, int64_t ld_mid,
                         float* feat, int64_t ld_feat, void* ws, vv_stream_t stream);
int vv_connector_pair_rows(const vv_connector* ac, const vv_connector* sem, const float* latent, int64_t ld_latent,
                           const float* semfeat, int64_t ld_feat, const int* active, float* out, int64_t ld_out,
                           int rows_out, int B, float* ws, vv_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * hipGraph capture of whatever the caller enqueues between begin/end on `stream`.
 * ------------------------------------------------------------------------------------------------------------ */
int vv_graph_begin(vv_stream_t stream);
int vv_graph_end(vv_stream_t stream, void** graph_exec_out);
int vv_graph_launch(void* graph_exec, vv_stream_t stream);
int vv_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------------------------------------------------
 * Per-launch timing of vv_linear with HIP events recorded on the launch stream (eager mode only, never during
 * graph capture).  vv_prof_begin arms it; vv_prof_end synchronises and aggregates by (m, n, k, dual, wdt).
 * The 3..8-row launches the composites make themselves (not through vv_linear) are recorded only for a
 * descriptor that carries VV_WQ_FRAG4, under the dtype they stream (VV_MXFP4_FRAG, or VV_BF16 for a matrix
 * without a copy); without the bit the record is what it always was.  The record list is locked: a row
 * batch's lanes call vv_linear from threads of their own.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vv_prof_entry { int m, n, k, dual, wdt, count; double total_ms; } vv_prof_entry;
int vv_prof_begin(int max_records);
int vv_prof_end(vv_prof_entry* out, int max_out, int* n_out);

/* ------------------------------------------------------------------------------------------------------------
 * vv_nf4_import — one matrix of a pre-quantized bitsandbytes 4-bit NF4 checkpoint (functional.quantize_4bit storage, QuantState.as_dict)
 * into the engine's layouts, in one pass over its packed bytes.  Load time only.
 *   packed:  ceil(n * k / 2) bytes over the row-major flattened [n, k] weight; element 2 i is the HIGH nibble of byte i, 2 i + 1 the low one
 *   absmax:  one scale per `blocksize` consecutive flattened elements (blocks may straddle rows): fp32 [nblocks], or with double quantisation
 *            (nested_absmax != NULL) uint8 codes [nblocks] decoded as (nested_map[code] * nested_absmax[b / nested_blocksize]) + nested_offset
 *   value:   bf16_rne(quant_map[code] * absmax[j / blocksize]) in fp32, each operation rounded on its own (no FMA contraction)
 * Writes rows row0 .. row0 + n - 1 of the destination (a fused [q|k|v] matrix takes q, k and v as three calls), which has rows_total rows:
 *   w:              bf16 [rows_total][ldw] row-major (ldw >= k)
 *   cq / cs:        optional (both or neither) VV_NF4 companion of the whole destination (codes and block absmax, the vv_linear layouts above,
 *                   ceil(rows_total / 4) * ceil(k / 512) * 1024 bytes and * 32 floats, zeroed by the caller: padding stays code 0 / scale 0).
 *                   Only when the companion holds the file's numbers exactly: k % 64 == 0, blocksize % 64 == 0 and k % blocksize == 0 (a block of
 *                   128 or 256 becomes 2 or 4 64-blocks repeating one scale); anything else with cq / cs is VV_E_ARG.
 * ------------------------------------------------------------------------------------------------------------ */
typedef struct vv_nf4_src {
  const uint8_t* packed;
  const void* absmax;            /* fp32, or uint8 codes when nested_absmax != NULL */
  const float* quant_map;        /* [16] */
  const float* nested_absmax;    /* [ceil(nblocks / nested_blocksize)] or NULL */
  const float* nested_map;       /* [256] (the stored dynamic map) */
  float nested_offset;
  int nested_blocksize;
  int n, k, blocksize;
} vv_nf4_src;
int vv_nf4_import(const vv_nf4_src* src, void* w, int64_t ldw, int row0, int rows_total, void* cq, float* cs, vv_stream_t stream);

/* The conv tokenizers' shape-specialised kernels (csrc/vv_conv_hot.hip): the table of call sites that have one, in the bit order of
 * vv_tune("conv_hot").  kind GEMV: a vv_linear call with exactly these m, n, k and epilogue operands (bf16 weights, no prologue, gate per
 * output column); kind ROW: the first FFN half of a one-row Block1D with C = k.  Copies up to cap entries, returns the table's length. */
#define VV_CONV_HOT_GEMV 0
#define VV_CONV_HOT_ROW 1
typedef struct vv_conv_hot_shape { const char* name; int kind, m, n, k, bias, gate, res; } vv_conv_hot_shape;
int vv_conv_hot_shapes(vv_conv_hot_shape* out, int cap);

/* struct sizes, for the ctypes mirror's self-check */
size_t vv_sizeof(const char* struct_name);

#ifdef __cplusplus
}
#endif
#endif /* VV_HIP_H */

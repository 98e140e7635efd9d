/* libldmae_hip -- C ABI of the MI355X (gfx950) kernels behind the LDMAE hot path.
 *
 * The reference (isno0907/ldmae) has NO native code and NO FFI: its seam for this path is the
 * Python module API (models/lightningdit.py, tokenizer/models_mae.py).  This header
 * is what a binding for that seam calls: one entry per fused region of the LightningDiT block /
 * VMAE encoder, each citing the reference lines whose arithmetic it replaces (paths relative to
 * /root/reference/LDMAE).  The ctypes binding lives in ldmae_amd/_lib.py, which PARSES THIS FILE at import for every prototype's
 * types: keep it to comments, preprocessor lines and plain C89 prototypes over int / long / long long / unsigned long long / float /
 * double / pointers (anything else makes the import raise).  INTEGRATION.md shows the stub a maintainer adds on the reference side.
 *
 * Conventions
 *  - plain device pointers + explicit sizes, no torch types; `stream` is a hipStream_t (NULL = default).
 *  - every call only ENQUEUES on `stream`: no allocation, no synchronisation; compute entry points keep no state
 *    between calls and are callable from the Python main thread and the autograd thread concurrently.
 *    Workspaces are caller-owned and used only inside the launches of the call that received them: two calls may share one
 *    workspace exactly when they are ordered on one stream (ldmae_amd/ops.py keys its scratch buffers by device, purpose AND stream).
 *    The only process-wide mutable state is the event list of the opt-in ldmae_prof_*
 *    timing hook (mutex-protected, off by default); per-device launch attributes (CU count, dynamic-LDS opt-in) are looked
 *    up per call.  A/B knobs and timeline stamps live in the separate diagnostic build only (csrc/probe/ldmae_diag.h).
 *  - return 0 on success, negative on error; ldmae_last_error() gives the thread-local message.
 *  - dtype codes select the activation type: LDMAE_F32 (parity path, exact-f32 MFMA) or LDMAE_BF16
 *    (throughput path, bf16 MFMA with f32 accumulation).  Residual stream, norms' statistics,
 *    modulation vectors, gradients of parameters and optimizer state are always f32.
 *  - "rows" M = batch * tokens, row-major, token-major activations [M, D].
 */
#ifndef LDMAE_HIP_H
#define LDMAE_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define LDMAE_OK 0
#define LDMAE_ERR_INVALID (-1)   /* bad argument / unsupported shape */
#define LDMAE_ERR_HIP (-2)       /* HIP runtime error at launch */

#define LDMAE_F32 0
#define LDMAE_BF16 1
/* fp16 activations: the TF32-CLASS forward path (round 5).  What the reference's drivers ask for with torch.backends.cuda.matmul.allow_tf32 = True
 * (inference.py:79, extract_features.py:2-3) is 10-bit-mantissa products with f32 accumulation; gfx950 has no TF32 MFMA, but fp16 has exactly
 * that mantissa at the bf16 rate, and the operands it is used for are O(1) (conversion saturates at +-65504).  Forward-only entry points:
 * ldmae_cast / ldmae_cast_weight (dst), ldmae_layernorm_fwd (out), ldmae_gemm_nt (dtype; epilogues BIAS / GATE_RES / BIAS_POS / BIAS_GELU; out
 * fp16 or f32; shapes of the whole-line kernel: K % 64 == 0, rows on 128-B lines), ldmae_attention_fwd_qkv (head_dim 16).  For VMAE pre-training
 * under fp16 autocast (engine_pretrain.py:51-57) also the backward: ldmae_gemm_nt(EPI_BIAS / EPI_GELU_BWD | LDMAE_EPI_F16_INF), ldmae_gemm_tn,
 * ldmae_attention_bwd_qkv (head_dim 16), ldmae_layernorm_bwd, ldmae_colsum, ldmae_gelu_fwd/bwd. */
#define LDMAE_F16 2
/* An entry point accepts exactly the dtype codes it has kernels for (stated with each prototype; f32 and bf16 where nothing is said).  Any
 * other code -- another of the three, or no code at all -- is refused with LDMAE_ERR_INVALID before anything is launched: no entry falls
 * back to the f32 kernel, which would run past the end of 16-bit buffers. */

/* GEMM epilogues */
#define LDMAE_EPI_BIAS 0       /* C = acc + bias (+ beta*C)                                   */
#define LDMAE_EPI_GATE_RES 1   /* y = acc + bias ; xout = xin + gate[b]*y  (gate NULL -> 1)    */
#define LDMAE_EPI_BIAS_POS 2   /* C = acc + bias + pos[m % rows_per_batch]  (patch-embed)      */
#define LDMAE_EPI_BIAS_GELU 3  /* C = gelu_erf(acc + bias)  (VMAE Mlp fc1), pre-activation to C2 */
#define LDMAE_EPI_SWIGLU 4     /* bf16 only: B = w12 [2Hs,K]; C = h12 [M,2Hs] = acc+bias (NULL: not stored -- forward-only), xout(as bf16*) = hid [M,Hs] = silu(x1)*x2 */
#define LDMAE_EPI_SWIGLU_BWD 5 /* bf16 only: acc = dhid [M,Hs]; xin(as bf16*) = h12 [M,2Hs]; C = dh12 [M,2Hs]; xout (optional) =
                                  [ceil(M/128)][2Hs] f32 partial column sums of dh12 as stored (bias gradient; caller sums the rows) */
#define LDMAE_EPI_GELU_BWD 6   /* C = dpre [M,N] = g * gelu_erf'(pre), g = acc (+ bias) rounded to out_dtype first; xin (read as out_dtype*) = pre [M, ldc]:
                                  the input gradient of fc2 with the GELU backward of the VMAE Mlp fused (models_mae.py:172: timm Mlp) */
#define LDMAE_EPI_QKV_ROPE 7   /* bf16 only, through ldmae_gemm_nt_qkv_rope: the qkv Linear with the QK-RMSNorm + RoPE front end of the attention fused
                                  (a wave's 64 output columns are one head of q, k or v) */
/* launch mode, or'ed into `epi` per call (bf16 GEMMs): one 256x256 tile per workgroup instead of one persistent workgroup per CU.  A
   data-parallel caller sets it while RCCL's collective kernels share the chip with backward (ldmae_amd/distributed.py); results are
   bitwise equal to the persistent launch */
#define LDMAE_EPI_TILE_LAUNCH 0x100
/* kernel form, or'ed into `epi` per call (bf16 GEMMs): keep the HALF-LINE kernel (64-B LDS rows, 16 x 64-B ring pieces: gemm_nt_persist_kernel)
   for a shape that the whole-line kernel (128-B LDS rows, gemm_nt_lines.hip -- the default wherever operand rows start on 128-B lines and
   K % 64 == 0) would take.  Same products in the same order: bitwise-equal results; tests and tools/bench_nt.py use it for A/B runs */
#define LDMAE_EPI_HALF_LINES 0x200
/* fp16 outputs (dtype LDMAE_F16), or'ed into `epi` per call: values beyond +-65504 become INFINITIES, as under torch's fp16 autocast -- what a
   gradient GEMM under a loss scaler wants (the scaler sees the non-finite gradient and skips the step).  Without the flag fp16 outputs SATURATE
   at +-65504 (the forward / TF32-class calls) */
#define LDMAE_EPI_F16_INF 0x400

const char* ldmae_last_error(void);
const char* ldmae_version(void);
const char* ldmae_arch(void);     /* "gfx950" */

/* ---- Linear layers -------------------------------------------------------------------------- */
/* C[M,N] = A[M,K] . B[N,K]^T with fused epilogue.  Replaces nn.Linear forward (lightningdit.py:59,
 * 64,68,88; swiglu_ffn.py:33,36; models_mae.py:125,127,133,143) and, with the [in,out] weight copy
 * as B, the input-gradient GEMM of the same layers.
 *   EPI_GATE_RES fuses `x = x + gate.unsqueeze(1) * branch(...)` (lightningdit.py:248-249):
 *   C (optional, dtype out_dtype) receives y for the backward pass, xin/xout are the f32 residual
 *   stream (may alias), gate is a [batch, gate_ld] f32 view, rows_per_batch = tokens per sample. */
int ldmae_gemm_nt(int dtype, int out_dtype, int epi, const void* A, int lda, const void* B, int ldb, void* C, int ldc,
                  int M, int N, int K, const float* bias, float beta, const float* xin, float* xout,
                  const float* gate, int gate_ld, int rows_per_batch, void* stream);
/* The qkv Linear of the DiT block (lightningdit.py:68) with q_norm / k_norm / RoPE (:70-74) applied in the GEMM's epilogue, head dim 64, bf16:
 *   qkv [B*N, 3*H*64] = A [B*N, K] . W [3*H*64, K]^T + bias as ldmae_gemm_nt(EPI_BIAS) writes it (the backward pass reads the pre-norm q / k rows; with
 *   store_raw_qk = 0 -- forward-only calls -- only the v third is written), and q2, k2 [B, H, N, 64] = what ldmae_qknorm_rope_fwd makes of the stored
 *   (bf16-rounded) q and k: bitwise the same values, without the pass that re-reads them.  wq = wk = NULL: RoPE only (use_qknorm = False).
 *   Covers B*N % 256 == 0, N % 128 == 0, K % 64 == 0, 128-B aligned operands (ldmae_gemm_nt_qkv_rope_ok says whether a shape is covered; the
 *   caller otherwise runs ldmae_gemm_nt + ldmae_qknorm_rope_fwd).  tile_launch: as LDMAE_EPI_TILE_LAUNCH. */
int ldmae_gemm_nt_qkv_rope_ok(int B, int N, int H, int hd, int K, int lda, int ldb);
int ldmae_gemm_nt_qkv_rope(const void* A, int lda, const void* W, int ldb, const float* bias, void* qkv, void* q2, void* k2, const float* wq,
                           const float* wk, const float* cos, const float* sin, int B, int N, int H, int hd, int K, float eps, int store_raw_qk,
                           int tile_launch, void* stream);
/* C[N,K] (f32) = beta*C + A[M,N]^T . B[M,K]: weight gradient of the same layers (contraction over
 * token rows, split over workgroups; partial slabs are summed in fixed order -> deterministic). */
int ldmae_gemm_tn_splits(int dtype, int M, int N, int K);
long ldmae_gemm_tn_workspace_bytes(int dtype, int M, int N, int K);
/* dbias (optional, [N] f32) = beta*dbias + column sums of A: the bias gradient of the same layer, fused. */
int ldmae_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, float* C, float* dbias, int M, int N, int K, float beta,
                  float* workspace, long workspace_bytes, void* stream);
/* out[N] (f32) = beta*out + column sums of X[M,N]: bias gradients. workspace >= ldmae_colsum_workspace_bytes */
long ldmae_colsum_workspace_bytes(int M, int N);
int ldmae_colsum(int dtype, const void* X, int ldx, int M, int N, float* out, float beta, float* workspace, void* stream);

/* f32 master weight [R,C] -> dst[R,C] (dtype) and, if dstT != NULL, dstT[C,R] (the [in,out] copy) */
int ldmae_cast_weight(int dst_dtype, const float* src, void* dst, void* dstT, int R, int C, void* stream);
int ldmae_cast(int src_dtype, int dst_dtype, const void* src, void* dst, long n, void* stream);
/* Thin f32 products with a contraction of K = 16 or 32 over M = batch * tokens rows -- the DiT's PatchEmbed at patch size 1
 * (lightningdit.py:309, 402: K = C * p * p) and dX of the FinalLayer's Linear (:270): HBM streaming, one pass over the big tensor.
 *   ldmae_thin_nt: out[M,N] (out_dtype) = T[M,K] . W[N,K]^T + bias[N] (+ pos[m % rows_per_batch, :] when pos != NULL); N % 4 == 0.
 *   ldmae_thin_tn: dW[N,K] = beta * dW + G[M,N]^T . T[M,K]; dbias[N] (may be NULL) = beta * dbias + column sums of G; partial sums per
 *                  512 rows, reduced in fixed order (deterministic); workspace >= ldmae_thin_tn_workspace_bytes(M, N, K). */
int ldmae_thin_nt(int out_dtype, const float* T, const float* W, const float* bias, const float* pos, void* out, int M, int N, int K,
                  int rows_per_batch, void* stream);
long ldmae_thin_tn_workspace_bytes(int M, int N, int K);
int ldmae_thin_tn(const float* G, const float* T, float* dW, float* dbias, int M, int N, int K, float beta, float* workspace,
                  long workspace_bytes, void* stream);
/* dst[i][0..n[i]) += src[i][0..n[i]) (f32) for `count` (<= 32) triples in one launch; dst / src / n are HOST arrays.  The host side uses it
 * to add a block's small parameter gradients into their .grad views in place of one AccumulateGrad add each (train_accum.py:236 backward). */
int ldmae_multi_add(int count, void* const* dst, const void* const* src, const long* n, void* stream);
/* `count` (<= 64) f32 device tensors of n_each elements each -> dst[count * n_each] in dst_dtype, one launch; srcs is a HOST array of device
 * pointers (16-B aligned; n_each % 8 == 0).  Used to stack the adaLN_modulation weights of all blocks (lightningdit.py:233-236) into the
 * [depth * 6D, D] operand of one GEMM. */
int ldmae_cast_stack(int dst_dtype, const void* const* srcs, int count, long n_each, void* dst, void* stream);

/* ---- adaLN-modulated RMSNorm (rmsnorm.py:51-77 + lightningdit.py:26-30) ----------------------- */
/* out = rmsnorm(x; w, eps) * (1 + scale[b]) + shift[b];  rstd[M] saved for backward.
 * shift/scale are [batch, mod_ld] f32 views (column slices of the adaLN output). */
int ldmae_rmsnorm_modulate_fwd(int out_dtype, const float* x, const float* w, const float* shift, const float* scale,
                               int mod_ld, void* out, float* rstd, int M, int D, int rows_per_batch, float eps, void* stream);
/* dx_accum = beta_x * dx_accum + d(x) (beta_x 0 or 1; 0 writes dx without reading it); dshift/dscale [batch, dmod_ld] = per-sample sums; dw[D] += sum (beta_w).  workspace from
 * ldmae_rmsnorm_modulate_bwd_workspace_bytes. */
long ldmae_rmsnorm_modulate_bwd_workspace_bytes(int M, int D, int rows_per_batch);
int ldmae_rmsnorm_modulate_bwd(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                               const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, float* dw,
                               float beta_w, int M, int D, int rows_per_batch, float* workspace, void* stream);
/* The same followed by the gated-residual backward (ldmae_gate_bwd) of the updated dx_accum, in one pass over the rows (the block's
 * norm2 backward feeds the attention branch's gate: lightningdit.py:247-248 read backwards): dy = dx_accum * gate[b] (in `dtype`),
 * dgate [B, dgate_ld] = sum_n dx_accum * y, dbias [D] = column sums of dy. */
long ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes(int M, int D, int rows_per_batch);
int ldmae_rmsnorm_modulate_bwd_gate(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                                    const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, float* dw,
                                    float beta_w, const void* y, const float* gate, int gate_ld, void* dy, float* dgate, int dgate_ld,
                                    float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream);
/* ldmae_rmsnorm_modulate_bwd_gate for a norm whose input row was never stored (the forward ran ldmae_res_rmsnorm_modulate_fwd): `x` is the
 * residual stream BEFORE the gated residual under the norm, and the row that was normalised is rebuilt in registers as x + gate[b] * y from
 * the y and gate the pass reads anyway.  Every output is bitwise what ldmae_rmsnorm_modulate_bwd_gate gives with that row materialised.
 * dtype LDMAE_BF16 only; workspace: ldmae_rmsnorm_modulate_bwd_gate_workspace_bytes. */
int ldmae_rmsnorm_modulate_bwd_gate_recompute(int dtype, const void* dout, const float* x, const float* w, const float* scale, int mod_ld,
                                              const float* rstd, float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld,
                                              float* dw, float beta_w, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                                              int dgate_ld, float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream);
/* The gated residual(s) of a block and the norm behind them in one pass over the rows (lightningdit.py:248-249): r = x + gate_a[b] * ya, and
 * r += gate_b[b] * yb when yb / gate_b are given; ya / yb are Linear outputs AS STORED in `dtype` (LDMAE_BF16 or LDMAE_F16), the gates [batch,
 * gate_ld] f32 views.  xout (optional, f32, not x) = r; out (optional, `dtype`) / rstd (optional) = ldmae_rmsnorm_modulate_fwd of r.  At least
 * one of xout / out.  Bitwise the LDMAE_EPI_GATE_RES epilogue (per residual) followed by ldmae_rmsnorm_modulate_fwd, without the f32 round
 * trip between them.  Every tensor 16-byte aligned, D % 4 == 0, M % rows_per_batch == 0. */
int ldmae_res_rmsnorm_modulate_fwd(int dtype, const float* x, const void* ya, const float* gate_a, int gate_a_ld, const void* yb,
                                   const float* gate_b, int gate_b_ld, float* xout, const float* w, const float* shift, const float* scale,
                                   int mod_ld, void* out, float* rstd, int M, int D, int rows_per_batch, float eps, void* stream);
/* The three entry points above for blocks built with use_rmsnorm=False: nn.LayerNorm(hidden, elementwise_affine=False, eps=1e-6) + modulate
 * (lightningdit.py:200-201,257; modulate :26-30).  y = (x - mean) * rstd * (1 + scale[b]) + shift[b]; rstd [M] = rsqrt(var + eps) is saved, the
 * backward recomputes the row mean from x.  No weight, no weight gradient; workspaces: ldmae_rmsnorm_modulate_bwd(_gate)_workspace_bytes. */
int ldmae_layernorm_modulate_fwd(int out_dtype, const float* x, const float* shift, const float* scale, int mod_ld, void* out, float* rstd,
                                 int M, int D, int rows_per_batch, float eps, void* stream);
int ldmae_layernorm_modulate_bwd(int dtype, const void* dout, const float* x, const float* scale, int mod_ld, const float* rstd, float* dx_accum,
                                 float beta_x, float* dshift, float* dscale, int dmod_ld, int M, int D, int rows_per_batch, float* workspace,
                                 void* stream);
int ldmae_layernorm_modulate_bwd_gate(int dtype, const void* dout, const float* x, const float* scale, int mod_ld, const float* rstd,
                                      float* dx_accum, float beta_x, float* dshift, float* dscale, int dmod_ld, const void* y, const float* gate,
                                      int gate_ld, void* dy, float* dgate, int dgate_ld, float* dbias, int M, int D, int rows_per_batch,
                                      float* workspace, void* stream);

/* ---- attention front end (lightningdit.py:68-74; rmsnorm.py on head_dim; pos_embed.py:38-42,135) */
/* qkv [B,N,3,H,hd] -> q,k = rope(rmsnorm(.)*w) and v, each [B,H,N,hd]. cos/sin [N,hd] f32.
 * wq = wk = cos = sin = NULL: plain head-major relayout (VMAE attention has no QK-norm / RoPE, models_mae.py:133-134).
 * wq = wk = NULL with cos / sin given: RoPE only -- the block built with use_qknorm=False, q_norm = k_norm = nn.Identity
 * (lightningdit.py:60-61,69; the reference's configs/celeba_hq/lightningdit_b_vmae_f8d16_cfg.yaml:30); backward: the rotation's adjoint, qkv /
 * dwq / dwk may be NULL.
 * v = NULL (fwd) / dv = NULL (bwd), forms with RoPE only: v stays in the packed buffer (see ldmae_attention_fwd_pv / _bwd_pv);
 * the backward then reads dv from the v slot of dqkv for the bias-gradient sums and leaves it in place. */
int ldmae_qknorm_rope_fwd(int dtype, const void* qkv, const float* wq, const float* wk, const float* cos, const float* sin,
                          void* q, void* k, void* v, int B, int N, int H, int hd, float eps, void* stream);
long ldmae_qknorm_rope_bwd_workspace_bytes(int B, int N, int H, int hd);
/* dbias_hqd (optional, [H][3][hd] f32): column sums of dqkv as stored = bias gradient of the qkv Linear, in (head, q|k|v, d) order */
int ldmae_qknorm_rope_bwd(int dtype, const void* dq, const void* dk, const void* dv, const void* qkv, const float* wq,
                          const float* wk, const float* cos, const float* sin, void* dqkv, float* dwq, float* dwk, float beta_w,
                          float* dbias_hqd, int B, int N, int H, int hd, float eps, float* workspace, void* stream);

/* Standalone 2-D RoPE, the callable form of VisionRotaryEmbeddingFast.forward (pos_embed.py:135; rotate_half :38-42):
 * out[r,:] = t[r,:]*cos[r % N,:] + rotate_half(t[r,:])*sin[r % N,:] on [rows, hd] (rows = anything x N).  transposed = 1: the adjoint
 * (backward).  The LightningDiT block does not use it: there the rotation is fused into ldmae_qknorm_rope_fwd / _bwd. */
int ldmae_rope(int dtype, const void* t, const float* cos, const float* sin, void* out, long rows, int N, int hd, int transposed,
               void* stream);

/* ---- attention core (F.scaled_dot_product_attention, lightningdit.py:76-80; manual softmax attention
 *      models_mae.py:135-141).  q,k,v [B,H,N,hd]; o [B,N,H*hd]; lse [B,H,N] f32 (natural log). */
int ldmae_attention_fwd(int dtype, const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int N, int hd,
                        float scale, void* stream);
/* N is arbitrary (the last 64-row tile of a sweep may be ragged: its missing rows are masked to -inf before the exponential).
 * delta: [2][B,H,NP] f32 workspace, NP = N rounded up to a multiple of 64 (bf16: -rowsum(dO*O) | -lse*log2(e), the initial accumulators
 * of the dK/dV pass; f32: slot 0 = rowsum(dO*O), first B*H*N floats); dq,dk,dv [B,H,N,hd]; do_ [B,N,H*hd] */
int ldmae_attention_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* do_, const float* lse,
                        void* dq, void* dk, void* dv, float* delta, int B, int H, int N, int hd, float scale, void* stream);

/* The same on the PACKED token-major qkv [B,N,3,H,hd] that the qkv Linear writes (bf16; the forward also f32 at head_dim 16): the VMAE blocks have no QK-norm / RoPE
 * between the Linear and the attention (models_mae.py:133-141), so q / k / v are read, and dq / dk / dv written, in place (no head-major
 * relayout passes).  dqkv [B,N,3,H,hd]. */
int ldmae_attention_fwd_qkv(int dtype, const void* qkv, void* o, float* lse, int B, int H, int N, int hd, float scale, void* stream);
/* ldmae_attention_fwd_qkv with a static softmax shift per (batch, head) (see ldmae_attention_fwd_pv_bounded): qk_max2 [B*H][2] f32 on the
 * device = (max_i |q_i|^2, max_j |k_j|^2) over the head's rows as stored (first value 0: each query's own norm is used); heads / waves whose
 * bound exceeds 50 keep the running maximum.  The
 * tiled VMAE encoder's q | k | v kernel produces the maxima as it writes the rows. */
int ldmae_attention_fwd_qkv_bounded(int dtype, const void* qkv, void* o, float* lse, const float* qk_max2, int B, int H, int N, int hd,
                                    float scale, void* stream);
/* qk_max2 [B*H][2] = (0, max_j |k_j|^2) from one pass over the k slots of a packed bf16 qkv: a first value of 0 makes the bounded kernel use
 * each query's own norm.  One extra pass over a third of qkv: pays for long sequences (the 1024-token VMAE decoder), not for short ones. */
int ldmae_k_norm_max(const void* qkv, float* qk_max2, int B, int N, int H, int hd, void* stream);
int ldmae_attention_bwd_qkv(int dtype, const void* qkv, const void* o, const void* do_, const float* lse, void* dqkv, float* delta,
                            int B, int H, int N, int hd, float scale, void* stream);

/* Mixed form for the LightningDiT block (bf16 only): q / k (dq / dk) head-major as QK-norm + RoPE produce them, v read from -- and dv
 * written into -- the v slot of the packed token-major qkv / dqkv [B,N,3,H,hd].  Pair with ldmae_qknorm_rope_fwd(v = NULL) and
 * ldmae_qknorm_rope_bwd(dv = NULL): v never gets a head-major copy. */
int ldmae_attention_fwd_pv(int dtype, const void* q, const void* k, const void* qkv, void* o, float* lse, int B, int H, int N, int hd,
                           float scale, void* stream);
/* The same with a STATIC softmax shift: score_bound = one float on the device, a proven upper bound of |q . k| * scale * log2(e) over all
 * queries and keys.  Bounds up to 50 make the kernel skip the running maximum (exact: every exponent lies in [-2 bound, 0]; -8 % of the
 * kernel at head_dim 64); larger ones fall back to the tracked form.  ldmae_qk_score_bound gives the bound for heads that went through
 * QK-RMSNorm + RoPE (lightningdit.py:66-80) from the two norm weights alone: hd * max|wq| * max|wk| * scale * log2(e) * 1.02 (the RoPE
 * tables must be rotations, cos^2 + sin^2 = 1, as models/pos_embed.py builds them). */
int ldmae_attention_fwd_pv_bounded(int dtype, const void* q, const void* k, const void* qkv, void* o, float* lse, const float* score_bound,
                                   int B, int H, int N, int hd, float scale, void* stream);
int ldmae_qk_score_bound(const float* wq, const float* wk, int hd, float scale, float* out, void* stream);
int ldmae_attention_bwd_pv(int dtype, const void* q, const void* k, const void* qkv, const void* o, const void* do_, const float* lse,
                           void* dq, void* dk, void* dqkv, float* delta, int B, int H, int N, int hd, float scale, void* stream);
/* ldmae_attention_bwd_pv + ldmae_qknorm_rope_bwd in one (bf16, head_dim 64 / 128): the QK-RMSNorm / RoPE backward (lightningdit.py:70-75
 * read backwards) runs in the epilogues of the dQ and dK/dV kernels, dq / dk are never written head-major.  dqkv [B,N,3,H,hd] complete;
 * dwq, dwk [hd] norm-weight gradients; dbias [3*H*hd] = column sums of dqkv (the qkv Linear's bias gradient).
 * wq = wk = dwq = dwk = NULL: RoPE adjoint only in the epilogues (use_qknorm=False, see ldmae_qknorm_rope_fwd). */
long ldmae_attention_bwd_pv_qknorm_workspace_bytes(int B, int H, int N, int hd);
int ldmae_attention_bwd_pv_qknorm(int dtype, const void* q, const void* k, const void* qkv, const void* o, const void* do_, const float* lse,
                                  const float* wq, const float* wk, const float* cos, const float* sin, float eps, void* dqkv, float* dwq,
                                  float* dwk, float* dbias, float* workspace, int B, int H, int N, int hd, float scale, void* stream);

/* ---- SwiGLU (swiglu_ffn.py:34-35) ------------------------------------------------------------ */
int ldmae_swiglu_fwd(int dtype, const void* h12, void* hid, int M, int Hs, void* stream);
int ldmae_swiglu_bwd(int dtype, const void* dhid, const void* h12, void* dh12, int M, int Hs, void* stream);

/* ---- gated residual backward (lightningdit.py:248-249): dy = dxout * gate[b]; dgate[b] = sum_n dxout*y;
   dbias (optional, [D]) = column sums of dy as stored = bias gradient of the branch's output Linear (proj / w3) */
long ldmae_gate_bwd_workspace_bytes(int M, int D, int rows_per_batch);
int ldmae_gate_bwd(int dtype, const float* dxout, const void* y, const float* gate, int gate_ld, void* dy, float* dgate,
                   int dgate_ld, float* dbias, int M, int D, int rows_per_batch, float* workspace, void* stream);

/* ---- embedders (lightningdit.py:109-137, 152-169) -------------------------------------------- */
int ldmae_timestep_embedding(const float* t, float* out, int B, int dim, float max_period, void* stream);
int ldmae_silu_fwd(int out_dtype, const float* x, void* out, long n, void* stream);
int ldmae_silu_bwd(const float* dy, const float* x, float* dx, long n, void* stream);   /* dx = dy * silu'(x) */
/* out[b] = table[drop[b] ? num_classes : y[b]]; drop may be NULL */
int ldmae_label_embed_fwd(const float* table, const long long* y, const unsigned char* drop, float* out, int B, int D,
                          int num_classes, void* stream);
/* dtable[rows,D] += scatter of dout (deterministic: one workgroup per table row, fixed b order) */
int ldmae_label_embed_bwd(const float* dout, const long long* y, const unsigned char* drop, float* dtable, int B, int D,
                          int num_classes, int rows, void* stream);

/* ---- optimizer (train_accum.py:121,240 AdamW; :336-347 EMA) ---------------------------------- */
/* one pass over flat f32 buffers: AdamW(lr,b1,b2,eps,wd) on p with grad g (scaled by grad_scale), then
 * ema = decay*ema + (1-decay)*p.  step >= 1. */
int ldmae_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long n, int step, double lr, double beta1,
                    double beta2, double eps, double weight_decay, double ema_decay, double grad_scale, void* stream);
int ldmae_ema_only(float* ema, const float* p, long n, double ema_decay, void* stream);
/* Power-function EMA tracks for post-hoc EMA reconstruction (Karras et al. 2024, section 3), in the AdamW pass.
 * p, m, v and ema are written exactly as ldmae_adamw_ema writes them (same expressions, same order: bit for bit).
 * Each of the ntracks (1..4) slabs t0..t3 then takes  e <- e + c (theta - e)  in f32, theta = the parameter after this
 * step's update, c_k = 1 - beta_k(t) = -expm1((gamma_k + 1) log1p(-1/t)) computed by the caller in f64 and rounded to
 * f32 here.  c_k == 1 (t = 1) stores theta and does NOT read the slab.  0 < c_k <= 1.  Any n; any base alignment (all
 * slabs congruent modulo 16 bytes use 16-byte accesses between a scalar head and a scalar tail). */
int ldmae_adamw_ema_tracks(float* p, const float* g, float* m, float* v, float* ema, long n, int step, double lr, double beta1,
                           double beta2, double eps, double weight_decay, double ema_decay, double grad_scale, int ntracks,
                           float* t0, float* t1, float* t2, float* t3, double c0, double c1, double c2, double c3, void* stream);
/* the same track update alone, for parameters the optimizer does not touch (the frozen tail: pos_embed) */
int ldmae_ema_tracks_only(const float* p, long n, int ntracks, float* t0, float* t1, float* t2, float* t3, double c0, double c1,
                          double c2, double c3, void* stream);
/* Combination of snapshots: acc[i] += coef * x[i] in f64 (coefficients of both signs), then out[i] = (float)acc[i]. */
int ldmae_snapshot_accumulate(double* acc, const float* x, long n, double coef, void* stream);
int ldmae_snapshot_finish(float* out, const double* acc, long n, void* stream);

/* ---- VMAE masked-token encoder (tokenizer/models_mae.py) ------------------------------------- */
/* random_masking (:472-497) on caller-supplied noise[N,L] f32: stable ascending argsort (ties -> lower
 * index first).  ids_restore i64 [N,L], mask f32 [N,L], ids_keep i64 [N,keep]. L <= 4096. */
int ldmae_random_masking(const float* noise, long long* ids_restore, float* mask, long long* ids_keep, int N, int L, int keep,
                         void* stream);
/* Patch-embed operand of the kept tokens only (inference; the mask depends on the noise alone, :472-497, so it can be applied BEFORE the
 * embedding conv of :502): tok [N*keep, C*p*p] (dtype tok_dtype) = the pixels of patch ids[n,j] of img [N,C,S,S] in the conv weight's
 * (c, i, j) order; posg [N*keep, D] f32 = pos[ids[n,j], :].  ldmae_gemm_nt(EPI_GATE_RES, xin = posg, gate = NULL) then gives the same bits
 * as embedding every patch and gathering. */
int ldmae_patch_gather(int tok_dtype, const float* img, const long long* ids, const float* pos, void* tok, float* posg, int N, int keep,
                       int C, int S, int p, int D, void* stream);
/* Latent-dataset prologue on the device, per batch (reference: datasets/img_latent_dataset.py:79-93 does it per item on the host; the shards
 * are written by extract_features.py:163-212).  sample = 1: moments [B, 2C, HW] f32 (mean | logvar) and noise [B, C, HW] ->
 * out[b,c,:] = ((mean + exp(0.5 * clamp(logvar, -30, 20)) * noise) - lat_mean[c]) / lat_std[c] * multiplier; sample = 0: moments is the
 * plain latent [B, C, HW] and noise is ignored.  lat_mean / lat_std [C] (latents_stats.pt) or both NULL (latent_norm off).  HW % 4 == 0. */
int ldmae_latent_prologue(const float* moments, const float* noise, const float* lat_mean, const float* lat_std, float multiplier,
                          float* out, int B, int C, int HW, int sample, void* stream);
/* Training transform of the packed image input on the device, per batch (datasets/packed_images.py; the host counterpart is
 * vmae_pretrain.RandomResizedCropFlip per item): crop, antialiased bicubic resize to S x S, horizontal flip, ToTensor and Normalize in one launch.
 * SOURCE.  Sample b reads the ch x cw crop at (top, left) of the h x w x 3 uint8 image (HWC, rows of 3 w bytes, no padding) at blob + offset[b];
 *   offset [B] i64 and geom [B, 8] i32 = (h, w, top, left, ch, cw, flip, 0) are DEVICE tables.  Any byte offset is accepted.
 * RESAMPLING.  PIL's crop(box).resize((S, S), BICUBIC): separable, horizontal pass then vertical, Keys cubic with a = -0.5, antialiased.  Per axis,
 *   input size n (cw, then ch): scale = n / S, fs = max(scale, 1), support = 2 fs; output index i has center = (i + 0.5) scale, taps
 *   x in [max(int(center - support + 0.5), 0), min(int(center + support + 0.5), n)) and weights cubic((x - center + 0.5) / fs) divided by their sum.
 *   Taps are clipped at the CROP BOX, not at the image: a pixel outside the box has no influence.  The tap count grows with scale without limit.
 * ARITHMETIC.  f32 throughout.  Tap bounds and the numerator / denominator of a weight's argument are formed in integers (exact), the argument
 *   is their f32 quotient; weights are normalised by their f32 sum taken in ascending tap order; each output is an ascending fma chain.  The
 *   horizontal result is clamped to [0, 255], then the vertical result is; nothing is rounded to integers (PIL rounds to 8 bits after each pass:
 *   the result differs from PIL's by at most (0.5 sum|w_v| + 0.5) / 255 of the pixel range).  out = (v / 255 - mean) / std
 *   with true divisions, each operation rounded once; out_bf16 = 1 stores that f32 value rounded to nearest even.  flip != 0 mirrors the columns.
 * MEMORY.  Only bytes inside [blob, blob + blob_bytes) are read: the kernel trusts its tables (ops.crop_resize_flip checks the host copy), and a
 *   row that fails the range check (box outside the image, image outside the blob, a crop side above 16384, h or w above 2^24) leaves its sample unwritten.  out
 *   [B, 3, S, S] f32 or bf16.  No atomics; the grid is a function of (B, S) alone; two launches give the same bits.
 * LDMAE_ERR_INVALID: B < 1, S < 1 or S > 16384, std == 0, a null pointer, an empty blob. */
int ldmae_crop_resize_flip_u8(const unsigned char* blob, long blob_bytes, const long* offset, const int* geom, void* out, int out_bf16, int B,
                              int S, float mean, float std, void* stream);
/* out[n,j,:] = x[n, ids[n,j], :]  (torch.gather on dim 1, :486); bwd scatters (ids unique per n) */
int ldmae_gather_rows(const float* x, const long long* ids, float* out, int N, int L, int keep, int D, void* stream);
int ldmae_scatter_rows(const float* dout, const long long* ids, float* dx, int N, int L, int keep, int D, void* stream);
/* Decoder input of the pre-training step (models_mae.py:536-541: cat([x, mask_token.repeat]) -> gather(ids_restore) -> + decoder_pos_embed) in
 * one pass: out[b,l,:] = (ids_restore[b,l] < keep ? x[b, ids_restore[b,l], :] : mask_token[:]) + pos[l,:].  x [B,keep,D], out [B,L,D] f32.
 * Backward: dx [B,keep,D] = the kept rows of dout (ids_restore[b,:] is a permutation), dmask_token [D] = column sums of the other rows. */
int ldmae_restore_tokens(const float* x, const float* mask_token, const float* pos, const long long* ids_restore, float* out, int B, int L,
                         int keep, int D, void* stream);
long ldmae_restore_tokens_bwd_workspace_bytes(int B, int L, int D);
int ldmae_restore_tokens_bwd(const float* dout, const long long* ids_restore, float* dx, float* dmask_token, int B, int L, int keep, int D,
                             float* workspace, void* stream);
/* The whole encoder stack after the gather -- nblocks x Block (models_mae.py:149-187) + the closing LayerNorm (:369, 521) -- as ONE kernel
 * for the shipped geometry at mask_ratio 0.75 (tokens = 256 kept tokens per image, dim 192, 12 heads, hidden 768; anything else returns
 * LDMAE_ERR_INVALID: use the per-layer entry points).  Inference only, bf16 MFMA, f32 residual stream held in registers: one workgroup
 * per image, activations never leave the CU.  x, out [B, tokens, dim] f32.  blob: ldmae_vmae_encoder_blob_bytes(nblocks) bytes of
 * weights as pre-arranged MFMA operand fragments in order of use (layout: csrc/vmae_fused.hip; packer: tokenizer/fused_encoder.py). */
long ldmae_vmae_encoder_blob_bytes(int nblocks);
int ldmae_vmae_encoder_fwd(const float* x, float* out, const void* blob, int B, int tokens, int dim, int heads, int hidden, int nblocks,
                           float eps, void* stream);
/* The same stack on sequences of SEVERAL whole 256-token tiles per image (tokens % 256 == 0; the docking encoder `_encode` runs all 1024
 * patches: models_mae.py:819-833): the same blob, three launches per block -- LayerNorm + q|k|v of a tile (tokens on the lanes, weights
 * through the LDS ring) -> ldmae_attention_fwd_qkv on the packed qkv -> proj + residual + LayerNorm + MLP + residual of a tile with the
 * residual stream in registers.  workspace: ldmae_vmae_encoder_fwd_tiled_workspace_bytes(B, tokens) bytes, 16-B aligned (qkv, attention
 * output, lse).  x may equal out. */
long ldmae_vmae_encoder_fwd_tiled_workspace_bytes(int B, int tokens);
int ldmae_vmae_encoder_fwd_tiled(const float* x, float* out, const void* blob, void* workspace, int B, int tokens, int dim, int heads,
                                 int hidden, int nblocks, float eps, void* stream);
/* the TF32-class form of the same call (fp16 operands = TF32's mantissa; the blob packed in fp16, same layout and size): what f32 docking calls
 * run while torch.backends.cuda.matmul.allow_tf32 is set (inference.py:79, extract_features.py:2-3) */
int ldmae_vmae_encoder_fwd_tiled_f16(const float* x, float* out, const void* blob, void* workspace, int B, int tokens, int dim, int heads,
                                     int hidden, int nblocks, float eps, void* stream);
/* LayerNorm with affine (models_mae.py:163,171,369; eps 1e-6).  mean/rstd [M] saved. */
int ldmae_layernorm_fwd(int out_dtype, const float* x, const float* w, const float* b, void* out, float* mean, float* rstd,
                        int M, int D, float eps, void* stream);
long ldmae_layernorm_bwd_workspace_bytes(int M, int D);
int ldmae_layernorm_bwd(int dtype, const void* dout, const float* x, const float* w, const float* mean, const float* rstd,
                        float* dx_accum, float* dw, float* db, float beta_w, int M, int D, float* workspace, void* stream);
/* the same with a second output: dx_cast [M,D] (bf16 / fp16 = dtype; NULL: none) = dx_accum AFTER the update, rounded -- the operand of the
 * next Linear's backward in a ViT block (saves the separate cast pass over the f32 residual gradient: 0.2 GB read per block at 256 images) */
int ldmae_layernorm_bwd_cast(int dtype, const void* dout, const float* x, const float* w, const float* mean, const float* rstd,
                             float* dx_accum, void* dx_cast, float* dw, float* db, float beta_w, int M, int D, float* workspace, void* stream);
/* exact-erf GELU (timm Mlp act, models_mae.py:172) */
int ldmae_gelu_fwd(int dtype, const void* x, void* out, long n, void* stream);
int ldmae_gelu_bwd(int dtype, const void* dout, const void* x, void* dx, long n, void* stream);
/* nn.GELU(approximate="tanh"): the timm Mlp of a LightningDiT block built with use_swiglu=False (lightningdit.py:208,219-224); f32 / bf16 */
int ldmae_gelu_tanh_fwd(int dtype, const void* x, void* out, long n, void* stream);
int ldmae_gelu_tanh_bwd(int dtype, const void* dout, const void* x, void* dx, long n, void* stream);
/* 3x3 / stride 1 / pad 1 convolution on [B,C,H,W] f32 (conv_decoder_pred.conv_smoother, models_mae.py:254,275) */
int ldmae_conv3x3(const float* x, const float* w, const float* b, float* out, int B, int C, int H, int W, void* stream);
/* its backward (VMAE pre-training trains the smoother, engine_pretrain.py:51-76): dx (optional) [B,C,H,W], dw [C,C,3,3], db [C]; C = 3 */
long ldmae_conv3x3_bwd_workspace_bytes(int C);
int ldmae_conv3x3_bwd(const float* dout, const float* x, const float* w, float* dx, float* dw, float* db, int B, int C, int H, int W,
                      float* workspace, void* stream);

/* The masked / visible reconstruction loss of forward_loss (models_mae.py:733-754) in IMAGE space: pred_img = the smoothing conv's output
 * [B,C,H,W] f32, imgs the input images, mask [B, (H/p)*(W/p)] f32 (1 = masked).  fwd: partials [ldmae_mae_loss_groups(B*C*H*W)][2] =
 * per-workgroup (sum over masked patches' pixels of d^2, the same over visible ones); the caller adds the rows and divides by p*p*C * patch
 * count.  bwd: dpred_img = 2 d (coef[0] mask + coef[1] (1 - mask)), coef on the device.  norm_pix_loss targets stay in torch. */
long ldmae_mae_loss_groups(long elements);
int ldmae_mae_loss_fwd(const float* pred_img, const float* imgs, const float* mask, float* partials, int B, int C, int H, int W, int p, void* stream);
int ldmae_mae_loss_bwd(const float* pred_img, const float* imgs, const float* mask, const float* coef, float* dpred_img, int B, int C, int H, int W,
                       int p, void* stream);

/* ---- FID evaluation: pytorch-fid's Inception-v3 (reference tools/calculate_fid.py:64-425), NHWC f32 -------------------------------
 * conv2d: implicit-GEMM convolution on the exact-f32 MFMA.  x [B, H, W, ldx] read at channels [xoff, xoff + Cin); w [Cout, kh, kw, Cin]
 * (K = kh*kw*Cin contiguous per output channel); out [B, Ho, Wo, ldo] written at channels [ooff, ooff + Cout), Ho = (H + 2 ph - kh) / sh + 1;
 * zero padding ph / pw; epilogue out = bias (may be NULL) + x (*) w, then max(., 0) when relu != 0 (BatchNorm folded into w and b).
 * pool2d: mode 0 = max over the in-image taps of a k x k window, mode 1 = average over them (count_include_pad=False); same channel-slice
 * conventions, C channels.  global_avgpool: out [B, C] = mean over HW pixels of x [B, HW, ldx] at channels [xoff, xoff + C).
 * fid_preprocess: uint8 [B, H, W, 3] RGB -> out [B, Ho, Wo, 3] = F.interpolate(img / 255, (Ho, Wo), bilinear, align_corners=False) * 2 - 1.
 * fid_stats_accumulate: sum[d] += sum_r (f[r, d] - shift[d]); cross[i, j] += sum_r (f[r, i] - shift[i]) (f[r, j] - shift[j]); f [n, D] f32,
 * sum / cross f64 on the device, accumulated across calls (the caller zeroes them once). */
int ldmae_conv2d_nhwc_f32(const float* x, int ldx, int xoff, const float* w, const float* bias, float* out, int ldo, int ooff, int B, int H, int W,
                          int Cin, int Cout, int kh, int kw, int sh, int sw, int ph, int pw, int relu, void* stream);
int ldmae_pool2d_nhwc_f32(int mode, const float* x, int ldx, int xoff, float* out, int ldo, int ooff, int B, int H, int W, int C, int k, int stride,
                          int pad, void* stream);
int ldmae_global_avgpool_nhwc_f32(const float* x, int ldx, int xoff, float* out, int B, int HW, int C, void* stream);
int ldmae_fid_preprocess(const unsigned char* img, float* out, int B, int H, int W, int Ho, int Wo, void* stream);
int ldmae_fid_stats_accumulate(const float* feats, int n, int D, const float* shift, double* sum, double* cross, void* stream);

/* ---- ADM evaluator: Inception Score, sFID, precision and recall (reference tools/evaluator.py), f32 --------------------------------
 * adm_preprocess: uint8 [B, H, W, 3] -> out [B, Ho, Wo, 3] = (TF1 legacy ResizeBilinear(img) - 128) / 128 (align_corners = False, no
 * half-pixel centres: src = dst * in / out, hi = min(lo + 1, in - 1); the rule is written out in csrc/adm_eval.hip).
 * adm_spatial_tap: out [B, HW * C] = x [B, HW, ldx] at channels [xoff, xoff + C), flattened (pixel, channel) = TF's NHWC reshape.
 * row_sqnorms_f32: out [M] = sum_d x[m, d]^2 of x [M, D], accumulated in f64, rounded to f32 once.
 * pairwise_logits: out [M, N] = u [M, D] . w [N, D]^T (no bias) on the exact-f32 MFMA.
 * knn_radii: d(i, j) = max(|x_i|^2 - 2 x_i.x_j + |x_j|^2, 0) over x [N, D] with norms [N]; radii [N, nk] = the value at sorted index
 * nhood[t] (0..7, self-distance included) of row i.  Columns are cut into nsplit ranges of whole 64-column tiles; partials (float,
 * knn_partials_bytes(N, nsplit) bytes) hold per-range lists.  The result does not depend on nsplit, bit for bit.
 * pr_flags: the same d between u [M, D] and v [N, D]; u_in [M, nk] = 1 where some j has d(i, j) <= rv[j, k], v_in [N, nk] = 1 where some
 * i has d(i, j) <= ru[i, k]; the caller zeroes u_in / v_in; only 1s are stored.
 * adm_softmax_is: p = softmax(logits [M, C]) in f32; h [M] = sum_c p log p (f64, 0 log 0 = 0); S [ceil(M / split), C] = sum of p over
 * each split of `split` consecutive rows (f64, fixed order).  workspace: adm_is_workspace_bytes(M, C, split) bytes.
 * kid_sums: the sums of the unbiased MMD^2 with the cubic polynomial kernel k(x, y) = (gamma x.y + coef0)^3 over S subsets of m rows each,
 * in one launch.  a [Na, D], b [Nb, D] f32; idx_a / idx_b [S, m] int32: row i of subset s is a[idx_a[s, i]] (b[idx_b[s, i]]), read through
 * the index, never gathered.  The kernel TRUSTS the tables: the caller checks every entry against [0, Na) / [0, Nb) on their host copy.
 * Per element g = the exact-f32 MFMA dot product, p = fmaf(gamma, g, coef0), p3 = (p * p) * p (each step rounded once to f32), added in
 * f64.  out [S, 3] f64 = (sum over i != j of k(a_i, a_j), sum over i != j of k(b_i, b_j), sum over all i, j of k(a_i, b_j)), i and j
 * positions in the subset.  Partials are one f64 per (s, sum, 128-row tile, 64-column tile), added in ascending (row tile, column tile)
 * order: no atomics, and the same bits for every nsplit.  workspace: kid_workspace_bytes(S, m) bytes.  Refused: m < 2, m > min(Na, Nb),
 * S < 1, S > 21845 (the grid's y extent holds 3 S).
 * ball_counts: d as in knn_radii between u [M, D] (norms nu, ONE radius column ru [M], squared distances as knn_radii writes them) and
 * v [N, D] (norms nv); counts [M] = #{ j : d(i, j) < ru[i] }, STRICTLY less (pr_flags keeps its <=).  partials (int,
 * ball_counts_partials_bytes(M, nsplit) bytes) hold one count per (row, column range, half tile); integer sums: nsplit cannot change them. */
int ldmae_adm_preprocess(const unsigned char* img, float* out, int B, int H, int W, int Ho, int Wo, void* stream);
int ldmae_adm_spatial_tap(const float* x, int ldx, int xoff, float* out, int B, int HW, int C, void* stream);
int ldmae_row_sqnorms_f32(const float* x, int M, int D, float* out, void* stream);
int ldmae_pairwise_logits(const float* u, int M, int D, const float* w, int N, float* out, void* stream);
long ldmae_knn_partials_bytes(int M, int nsplit);
int ldmae_knn_radii(const float* x, const float* norms, int N, int D, const int* nhood, int nk, int nsplit, float* partials, float* radii,
                    void* stream);
int ldmae_pr_flags(const float* u, const float* nu, const float* ru, int M, const float* v, const float* nv, const float* rv, int N, int D, int nk,
                   int nsplit, int* u_in, int* v_in, void* stream);
long ldmae_adm_is_workspace_bytes(int M, int C, int split);
int ldmae_adm_softmax_is(const float* logits, int M, int C, int split, void* workspace, double* h, double* S, void* stream);
long ldmae_kid_workspace_bytes(int S, int m);
int ldmae_kid_sums(const float* a, int Na, const float* b, int Nb, int D, const int* idx_a, const int* idx_b, int S, int m, float gamma,
                   float coef0, int nsplit, void* workspace, double* out, void* stream);
long ldmae_ball_counts_partials_bytes(int M, int nsplit);
int ldmae_ball_counts(const float* u, const float* nu, const float* ru, int M, const float* v, const float* nv, int N, int D, int nsplit,
                      int* partials, int* counts, void* stream);

/* ---- tokenizer evaluation: rFID, PSNR, SSIM and LPIPS (reference evaluate_tokenizer.py, models/lpips.py), f32 ----------------------
 * lpips_prep: input / target NCHW [B, 3, H, W] -> out NHWC [2B, H, W, 4] = (x - shift) / scale of LPIPS' ScalingLayer (shift -0.030, -0.088,
 * -0.188; scale 0.458, 0.448, 0.450); images 0..B-1 from input, B..2B-1 from target, channel 3 = 0.  out 16-byte aligned.
 * lpips_layer: f NHWC [2B, h, w, C] (C = 64, 128, 256 or 512), lin_w [C]; per pixel f^ = f / (sqrt(sum_c f^2) + 1e-10) of both halves and
 * d = sum_c lin_w[c] (f^_b - f^_(B+b))^2; out[b] += mean over the h * w pixels of d.  workspace: lpips_workspace_bytes(B, h, w) bytes.
 * ssim: per-image SSIM [B] of preds / target NCHW [B, C, H, W] as torchmetrics' StructuralSimilarityIndexMeasure with its defaults: inputs
 * clamped to [lo, hi], c1 = (0.01 data_range)^2, c2 = (0.03 data_range)^2, separable 11-tap Gaussian (sigma 1.5) of x, y, x^2, y^2, xy,
 * variances clamped at 0, the map cropped by 5 on every side and averaged over C (H - 10) (W - 10).  H, W >= 11.
 * workspace: ssim_workspace_bytes(B, C, H, W) bytes.
 * recon_quantize_psnr: decoded / ref NCHW [B, 3, H, W] -> dec8 / ref8 NHWC uint8 [B, H, W, 3] = (uint8) clamp(127.5 x + 128, 0, 255)
 * (truncation; multiply and add rounded separately) and sse[B] = exact sum over the 3 H W values of (dec8 - ref8)^2.
 * sse_u8: sse[B] = exact sum of (a - b)^2 over n uint8 values per image.  workspace of both: sse_workspace_bytes(B, pixels) bytes, 8-byte
 * aligned, pixels = H W (recon_quantize_psnr) or n (sse_u8).  Every per-image sum is two-stage and fixed-order: bitwise reproducible. */
int ldmae_lpips_prep(const float* input, const float* target, float* out, int B, int H, int W, void* stream);
long ldmae_lpips_workspace_bytes(int B, int h, int w);
int ldmae_lpips_layer(const float* f, const float* lin_w, float* out, int B, int h, int w, int C, void* workspace, void* stream);
long ldmae_ssim_workspace_bytes(int B, int C, int H, int W);
int ldmae_ssim(const float* preds, const float* target, float* out, int B, int C, int H, int W, float lo, float hi, float data_range,
               void* workspace, void* stream);
long ldmae_sse_workspace_bytes(int B, long pixels);
int ldmae_recon_quantize_psnr(const float* decoded, const float* ref, unsigned char* dec8, unsigned char* ref8, long long* sse, int B, int H,
                              int W, void* workspace, void* stream);
int ldmae_sse_u8(const unsigned char* a, const unsigned char* b, long long* sse, int B, long n, void* workspace, void* stream);

/* ---- LPIPS backward (stage 3 of train_ae.sh: decoder tuning with the perceptual loss), f32 NHWC, no atomics: bitwise reproducible ----
 * conv3x3_relu_dgrad_nhwc_f32: data gradient of y = relu(conv3x3(x, w) + b), stride 1, pad 1.  dy, y [B, H, W, Cy] (Cy % 4 == 0), w_rot
 * [Cx, 3, 3, Cy] with w_rot[ci][ky][kx][co] = w[co][2 - ky][2 - kx][ci]; dx [B, H, W, Cx] = conv3x3(dy * [y > 0], w_rot), overwritten.  The
 * mask is applied while the operand is gathered; the main loop is the forward conv's exact-f32 MFMA loop.
 * maxpool2x2_bwd_nhwc_f32: dx [B, H, W, C] from dy [B, H/2, W/2, C] and the pooled input x [B, H, W, C] (C % 4 == 0): dy goes to the window's
 * maximum, the first in row-major order on a tie; rows / columns past 2 floor(H/2), 2 floor(W/2) get 0; every element of dx is written.
 * lpips_layer_bwd: f [2B, h, w, C] and lin_w [C] as lpips_layer takes them, g [B] the gradient of the per-pair value; d_input / d_target
 * [B, h, w, C] receive the gradient to f's first / second half (null: not wanted; at least one).  accumulate != 0 adds into them (the tap's
 * buffer already holds the pool backward's gradient), else overwrites.  A pixel that is all zero in a half gets exactly 0 in that half.
 * lpips_prep_bwd: g NHWC [B, H, W, 4] -> out NCHW [B, 3, H, W] = g[..., c] / scale[c] (the ScalingLayer's backward). */
int ldmae_conv3x3_relu_dgrad_nhwc_f32(const float* dy, const float* y, const float* w_rot, float* dx, int B, int H, int W, int Cy, int Cx,
                                      void* stream);
int ldmae_maxpool2x2_bwd_nhwc_f32(const float* dy, const float* x, float* dx, int B, int H, int W, int C, void* stream);
int ldmae_lpips_layer_bwd(const float* f, const float* lin_w, const float* g, float* d_input, float* d_target, int B, int h, int w, int C,
                          int accumulate, void* stream);
int ldmae_lpips_prep_bwd(const float* g, float* out, int B, int H, int W, void* stream);

/* ---- LPIPS in 16 bits (models/lpips.py, precision="fp16"; csrc/lpips_f16.hip): the reference's autocast arithmetic without its loss scaler ----
 * The arithmetic contract.  FORWARD: every conv operand is fp16 (round to nearest even, saturating at +-65504 as ldmae_cast does); products are
 * exact in f32 and accumulated in f32 on v_mfma_f32_16x16x32_f16; bias is added in f32, ReLU applied, and the result rounded ONCE to fp16
 * (saturating) and stored as fp16 NHWC: activations between layers live in memory as fp16.  The max pool runs on fp16 (exact); the heads read the
 * fp16 taps and do all their arithmetic in f32.  BACKWARD: gradients stay f32 in memory; the data-gradient conv rounds both operands to bf16
 * (dy * [y > 0] at the fetch, w_rot once by the caller), accumulates in f32 on v_mfma_f32_16x16x32_bf16 and writes f32; the ReLU mask is y > 0 on
 * the stored fp16 activation.  bf16, not fp16: the gradient scales as 1 / (h w) and falls below fp16's smallest normal already at 33 x 47.
 * No split K, no atomics: summation order is fixed by the shape, the same bits run to run.
 * lpips_prep_f16: ldmae_lpips_prep's f32 arithmetic, then one rounding; out fp16 NHWC [2B, H, W, 8], channels 3 .. 7 zero.  out 16-B aligned.
 * conv3x3_relu_nhwc_f16: x fp16 [B, H, W, Cin] (Cin % 8 == 0), w fp16 [Cout, 3, 3, Cin], bias f32 [Cout] or NULL, out fp16 [B, H, W, Cout] =
 * fp16(max(conv + bias, 0)); stride 1, pad 1; any Cout, any B H W.  x, w 16-B aligned.
 * maxpool2x2_nhwc_f16: x fp16 [B, H, W, C] (C % 8 == 0, H, W >= 2) -> out fp16 [B, H/2, W/2, C]; the odd last row / column is dropped.
 * lpips_layer_f16 / lpips_layer_bwd_f16: ldmae_lpips_layer / ldmae_lpips_layer_bwd with f fp16; out, g, d_input, d_target f32, the same arithmetic.
 * conv3x3_relu_dgrad_nhwc_bf16: dy f32 [B, H, W, Cy] (Cy % 8 == 0), y fp16 of the same shape, w_rot bf16 [Cx, 3, 3, Cy], dx f32 [B, H, W, Cx],
 * overwritten.  dy, y, w_rot 16-B aligned.
 * maxpool2x2_bwd_nhwc_xf16: ldmae_maxpool2x2_bwd_nhwc_f32 with the pooled input x fp16; dy, dx f32.
 * lpips_prep_bwd_c8: g f32 NHWC [B, H, W, 8] (conv1_1's data gradient; channels 3 .. 7 are ignored) -> out NCHW [B, 3, H, W] = g[..., c] / scale[c]. */
int ldmae_lpips_prep_f16(const float* input, const float* target, void* out, int B, int H, int W, void* stream);
int ldmae_conv3x3_relu_nhwc_f16(const void* x, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout, void* stream);
int ldmae_maxpool2x2_nhwc_f16(const void* x, void* out, int B, int H, int W, int C, void* stream);
int ldmae_lpips_layer_f16(const void* f, const float* lin_w, float* out, int B, int h, int w, int C, void* workspace, void* stream);
int ldmae_conv3x3_relu_dgrad_nhwc_bf16(const float* dy, const void* y, const void* w_rot, float* dx, int B, int H, int W, int Cy, int Cx,
                                       void* stream);
int ldmae_maxpool2x2_bwd_nhwc_xf16(const float* dy, const void* x, float* dx, int B, int H, int W, int C, void* stream);
int ldmae_lpips_layer_bwd_f16(const void* f, const float* lin_w, const float* g, float* d_input, float* d_target, int B, int h, int w, int C,
                              int accumulate, void* stream);
int ldmae_lpips_prep_bwd_c8(const float* g, float* out, int B, int H, int W, void* stream);

/* ---- convolutional KL-VAE tokenizers (tokenizer/autoencoder.py: the LDM Encoder / Decoder), f32 NHWC, forward only -----------------------
 * groupnorm_stats: mean / rstd [B, G] of x [B, HW, C]: per (image, group) mean and rstd = 1 / sqrt(var + eps), biased variance over the
 * HW * (C / G) elements of the group; two passes (mean, then the mean of (x - mean)^2), blocked summation (csrc/conv_vae.hip).
 * groupnorm_apply: out = gamma (x - mean) rstd + beta, then y * sigmoid(y) when silu != 0.
 * conv3x3_vae: 3x3 implicit-GEMM convolution on the exact-f32 MFMA; x [B, H, W, Cin] (Cin % 4 == 0), w [Cout, 3, 3, Cin], out [B, Ho, Wo, Cout]
 * = conv + bias (may be NULL) + res (may be NULL; the output's shape).  mode PLAIN: stride 1, pad 1.  NORM_ACT: the operand is
 * groupnorm_apply(x) computed while it is gathered (mean / rstd [B, G], gamma / beta [Cin], silu as above), stride 1, pad 1; taps outside
 * the image contribute exactly 0.  DOWN: stride 2, zero pad right and bottom only, Ho = (H + 1 - 3) / 2 + 1.  UP: the operand is the
 * nearest-neighbour 2x enlargement of x, read at (y >> 1, x >> 1) and never stored; stride 1, pad 1, Ho = 2 H.  mean, rstd, gamma, beta, G
 * and silu are read in NORM_ACT only.
 * conv1x1_res: out [M, Cout] = x [M, Cin] w [Cout, Cin]^T + bias + res, the same epilogue on a 1x1 convolution.
 * softmax_rows: in place, s[r, :cols] = softmax(scale * s[r, :cols]) and s[r, cols:ld] = 0 (rows padded for the GEMM that follows). */
#define LDMAE_VAE_PLAIN 0
#define LDMAE_VAE_NORM_ACT 1
#define LDMAE_VAE_DOWN 2
#define LDMAE_VAE_UP 3
int ldmae_groupnorm_stats_nhwc_f32(const float* x, float* mean, float* rstd, int B, int HW, int C, int G, float eps, void* stream);
int ldmae_groupnorm_apply_nhwc_f32(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* out, int B,
                                   int HW, int C, int G, int silu, void* stream);
int ldmae_conv3x3_vae_nhwc_f32(int mode, const float* x, const float* w, const float* bias, const float* res, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, int G, int silu, float* out, int B, int H, int W, int Cin, int Cout,
                               void* stream);
int ldmae_conv1x1_res_nhwc_f32(const float* x, const float* w, const float* bias, const float* res, float* out, int M, int Cin, int Cout, void* stream);
int ldmae_softmax_rows_f32(float* s, int ld, int rows, int cols, float scale, void* stream);
/* The TF32-class form of the two convolutions (the rule of LDMAE_F16 above: the reference's drivers run these layers with allow_tf32, 10-bit
 * mantissa products with f32 accumulation).  The arithmetic contract: both operands of every product are rounded ONCE to fp16, round to nearest
 * even, saturating at +-65504 as ldmae_cast does; products are accumulated in f32 on the fp16 MFMA; bias and residual are added in f32 and
 * the output is f32.  The residual stream, the GroupNorm statistics and everything between kernels stay f32.  In NORM_ACT the operand is
 * fp16(silu(gamma (x - mean) rstd + beta)): normalise and SiLU in f32 exactly as in the f32 kernels, then one rounding; a tap outside the
 * frame is exactly 0 and bypasses the activation.  Summation order is fixed by the shape: the same bits run to run.
 * conv3x3_vae_nhwc_f16: modes, virtual-frame gather and epilogue of ldmae_conv3x3_vae_nhwc_f32.  w is fp16 [Cout, 3, 3, Cin], already packed
 * (ldmae_cast of the f32 pack).  x_dtype LDMAE_F32: x is f32 and is rounded while it is staged; LDMAE_F16: x is fp16 (what
 * groupnorm_apply_nhwc_f16out wrote), PLAIN mode only -- the two-pass form of norm-act, with results identical to the fused one.
 * Cin % 8 == 0 (a 16-byte fp16 fragment never straddles a tap); any Cout, any M.  x, w, gamma, beta 16-B aligned.
 * conv1x1_res_nhwc_f16: the same kernel with a 1x1 window; x f32 [M, Cin], w fp16 [Cout, Cin], Cin % 8 == 0.
 * groupnorm_apply_nhwc_f16out: ldmae_groupnorm_apply_nhwc_f32 writing fp16 [B, HW, C] (saturating, round to nearest even). */
int ldmae_conv3x3_vae_nhwc_f16(int mode, int x_dtype, const void* x, const void* w, const float* bias, const float* res, const float* mean,
                               const float* rstd, const float* gamma, const float* beta, int G, int silu, float* out, int B, int H, int W, int Cin,
                               int Cout, void* stream);
int ldmae_conv1x1_res_nhwc_f16(const float* x, const void* w, const float* bias, const float* res, float* out, int M, int Cin, int Cout, void* stream);
int ldmae_groupnorm_apply_nhwc_f16out(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, void* out, int B,
                                      int HW, int C, int G, int silu, void* stream);

/* ---- adaptive Dormand-Prince 5(4) ODE sampler (transport/integrators.py, sampling_method dopri5; csrc/ode.hip), f32 -----------------
 * The seven stage derivatives live in one slab k_slab[7][ld], ld % 4 == 0 and ld >= n (every row 16-byte aligned for any n); y, y1, y_mid,
 * out are dense [n], 16-byte aligned.  h, t, the error ratio and the norms are single floats in DEVICE memory: nothing here synchronises.
 * Every sum is two-stage and fixed-order (no atomics; the order depends on n only): bitwise reproducible.  partial: ode_partials(n) floats.
 * rk_stage: out = y + h * sum_{j < m} coef[j] * k_j, evaluated as acc = coef[0] * k_0; acc = fma(coef[j], k_j, acc) for j = 1 .. m - 1;
 * out = fma(h, acc, y).  coef is a HOST array of m floats (passed to the kernel by value), 1 <= m <= 7, h = *h_dev.  t_out != NULL: also
 * t_out[0 .. nt) = fma(ct, h, *t_dev), the time vector of the next model evaluation.
 * dopri5_finish: y1 = y + h * sum b_j k_j (the same operations as rk_stage with the tableau's last row, the zero weights skipped) and
 * *ratio_dev = sqrt(mean((h * sum e_j k_j / (atol + rtol * max(|y|, |y1|)))^2)) over all n elements; the error vector is never stored.
 * rms_norm_scaled: *out_dev = sqrt(mean((x / (atol + rtol * |y|))^2)), y = x when y_or_null is NULL.
 * dopri5_interp: out = the quartic through y0, y1, y_mid with slopes f0 = k_0, f1 = k_6, at x = (t_eval - *t0_dev) / *h_dev; exactly y0 at x = 0.
 * dopri5_advance (one thread): r = *ratio_dev; accepted when r <= 1; h' = h * (r == 0 ? 10 : min(10, max(0.9 / r^(1/5), r < 1 ? 1 : 0.2)));
 * t' = accepted ? t + h : t; writes status_dev[0..5] = {accepted, r, t, h, t', h'} (the record the host reads) and *t_dev = t', *h_dev = h'.
 * dopri5_initial_step (one thread): the Hairer-Norsett-Wanner starting step from d_dev = {d0, d1, d2 h0, h0}: phase 0 writes
 * h0 = (d0 < 1e-5 or d1 < 1e-5) ? 1e-6 : 0.01 d0 / d1 to *h_dev and d_dev[3]; phase 1 writes min(100 h0, (0.01 / max(d1, d2))^(1/5)). */
int ldmae_ode_partials(long n);
int ldmae_rk_stage_f32(const float* y, const float* k_slab, long ld, const float* coef, int m, const float* h_dev, float* out, long n,
                       const float* t_dev, float ct, float* t_out, int nt, void* stream);
int ldmae_dopri5_finish_f32(const float* y, const float* k_slab, long ld, const float* h_dev, float atol, float rtol, float* y1, float* partial,
                            float* ratio_dev, long n, void* stream);
int ldmae_rms_norm_scaled_f32(const float* x, const float* y_or_null, float atol, float rtol, float* partial, float* out_dev, long n, void* stream);
int ldmae_dopri5_interp_f32(const float* y0, const float* y1, const float* y_mid, const float* k_slab, long ld, const float* h_dev,
                            const float* t0_dev, float t_eval, float* out, long n, void* stream);
int ldmae_dopri5_advance(const float* ratio_dev, float* h_dev, float* t_dev, float* status_dev, void* stream);
int ldmae_dopri5_initial_step(float* d_dev, int phase, float* h_dev, void* stream);
/* Likelihood evaluation (transport.Sampler.sample_ode_likelihood: the probability-flow ODE on the augmented state (x, logp) with Hutchinson's
 * trace estimator), f32, no atomics, fixed summation order.
 * rademacher: out[i] = +1 or -1 from Philox4x32-10 (Salmon, Moraes, Dror & Shaw, SC'11) with key (seed low, seed high) and counter words
 * (counter low, counter high, v low, v high), v = i / 4: element i takes word i % 4 of block v, +1 when the word's top bit is set.
 * rowdot: out[r] = sum_j a[r, j] b[r, j] for B rows of m floats (a, b dense [B, m]; b == a gives the row sums of squares).  One fma chain per
 * thread over its elements of a 4096-element chunk of the row, the block sum of csrc/ode.hip, partial[r * ceil(m / 4096) + c], then one block
 * per row folds its chunks.  16-byte loads when every row start is aligned, element loads otherwise (another, equally fixed, order).
 * partial: ldmae_rowdot_partials(B, m) floats.
 * likelihood_finish: logp[b] = (c - sumsq[b] / 2) - delta[b], c = -m / 2 log(2 pi) from the host; every operation rounded once. */
int ldmae_rademacher_f32(float* out, long n, unsigned long long seed, unsigned long long counter, void* stream);
long ldmae_rowdot_partials(int B, long m);
int ldmae_rowdot_f32(const float* a, const float* b, float* out, int B, long m, float* partial, void* stream);
int ldmae_likelihood_finish_f32(const float* sumsq, const float* delta, float c, float* logp, int B, void* stream);
/* SDE sampler (transport.Sampler.sample_sde: Euler-Maruyama / Heun on the linear path), f32, 16-byte accesses, grid a function of n alone.
 * normal: out[i] = a standard normal from Philox4x32-10, key and counter words as rademacher (block v = i / 4).  Word w_j of the block gives
 * u_j = ((w_j >> 9) + 0.5) 2^-23 (exact in f32; strictly inside (0, 1)); Box-Muller on (u0, u1) and (u2, u3): r = sqrt(-2 ln u_a),
 * (r cos(2 pi u_b), r sin(2 pi u_b)); element i takes value i % 4 of its block.  |out[i]| <= sqrt(48 ln 2) = 5.77.
 * sde_combine: out = sum_{j < m} coef[j] in_j + noise_coef * z, m in 1..4 (coef: m host floats; in_j unused for j >= m), accumulated left to
 * right: coef[0] in_0 rounded, then one fma per further term, the noise term last.  noise_mode 0: no noise term; 1: z is a tensor; 2: z is the
 * draw normal(seed, counter), generated in the same pass and never stored (bit for bit what mode 1 gives on ldmae_normal_f32's output).
 * mean_out (or NULL) receives the sum without the noise term.  t_out (or NULL): t_out[0..nt) = t_next.  Every tensor 16-byte aligned
 * (t_out 4-byte).  out and mean_out may each BE one of the inputs or z (in place); a partial overlap is refused (LDMAE_ERR_INVALID), as is
 * out overlapping mean_out, or t_out overlapping anything. */
int ldmae_normal_f32(float* out, long n, unsigned long long seed, unsigned long long counter, void* stream);
int ldmae_sde_combine_f32(const float* in0, const float* in1, const float* in2, const float* in3, const float* coef, int m, const float* z,
                          float noise_coef, int noise_mode, unsigned long long seed, unsigned long long counter, float* out, float* mean_out,
                          long n, float t_next, float* t_out, int nt, void* stream);

/* ---- optional per-kernel timing hook used by bench.py for the roofline line ------------------- */
/* When enabled, ldmae_gemm_nt brackets each launch with HIP events on the launch stream. */
int ldmae_prof_enable(int on);
int ldmae_prof_collect(double* total_ms, double* total_flops, long* launches);   /* syncs the events; resets */
/* Launch counts by kernel family since the last reset, always on (one relaxed atomic add per entry-point call): which ARITHMETIC TYPE a
 * model's calls were dispatched to -- a bf16 forward that silently runs the f32 kernels (round 3: the VMAE decoder under autocast, 250 of
 * 304 ms) shows up as f32 counts.  counts[0..5] = NT GEMM bf16 / f32, TN GEMM bf16 / f32, attention (fwd or bwd entry) bf16 / f32;
 * counts[6..8] = NT GEMM / attention / TN GEMM in fp16 (the TF32-class forward path; VMAE pre-training under fp16 autocast).  n = how many to copy (<= 9).  reset != 0 zeroes them after the copy. */
#define LDMAE_COUNT_NT_BF16 0
#define LDMAE_COUNT_NT_F32 1
#define LDMAE_COUNT_TN_BF16 2
#define LDMAE_COUNT_TN_F32 3
#define LDMAE_COUNT_ATTN_BF16 4
#define LDMAE_COUNT_ATTN_F32 5
#define LDMAE_COUNT_NT_F16 6      /* round 5: the TF32-class (fp16) forward family */
#define LDMAE_COUNT_ATTN_F16 7
#define LDMAE_COUNT_TN_F16 8
int ldmae_launch_counts(long* counts, int n, int reset);

/* ---- MXFP8 sampling mode: block-scaled fp8 GEMMs for the DiT block (opt-in, forward-only) ----------
 * THE ARITHMETIC CONTRACT.
 *  MX block quantisation.  A row of length K (K % 128 == 0) is cut into blocks of 32 consecutive elements.  Per block: amax = max |x| =
 *   m * 2^x with m in [1, 2); scale exponent e = x - 8 if m <= 1.75, else x - 7 (the smallest e with amax * 2^-e <= 448: nothing
 *   saturates), clamped to [-127, 127], e = -127 for amax == 0; computed from the exponent and mantissa bits in integer arithmetic.  The
 *   scale is stored as the E8M0 byte e + 127 (0xFF is never produced), the elements as OCP e4m3fn (not fnuz) bytes: round-to-nearest-even
 *   of x * 2^-e (a multiplication by a power of two: exact).  +0 and -0 are one value.  Non-finite and f32-subnormal inputs: unspecified.
 *  Operands.  Weights are quantised from the f32 master weight along K (their input dimension); activations from the bf16 value that the
 *   bf16 path would have fed to the same GEMM.  The mode is "the bf16 forward with a quantiser in front of four GEMMs".
 *  Product.  Exact products of the dequantised values, accumulated in f32 on the scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4), the
 *   128-deep K-steps in order, no split-K: run-to-run bitwise reproducible.  Everything after the accumulator is the epilogue code of the
 *   bf16 kernels with its roundings.
 * The mode's effect on FID has not been measured.  It needs a trained checkpoint.
 *
 * q [M, K] e4m3 bytes and scales [M, K/32] E8M0 bytes, both row-major and dense, from rows of f32 or bf16 (src_dtype) `ld` elements apart. */
int ldmae_mx8_quantize(int src_dtype, const void* src, int ld, void* q, void* scales, int M, int K, void* stream);
/* The arithmetic of ldmae_rmsnorm_modulate_fwd with a bf16 output (RMSNorm weight w given; shift and / or scale may be NULL) up to and
 * including its bf16 rounding, quantised in the same kernel: q [M, D], scales [M, D/32] and rstd [M] (may be NULL) are bitwise what that
 * entry point followed by the quantiser writes.  D % 128 == 0, D <= 2048. */
int ldmae_rmsnorm_modulate_fwd_mx8(const float* x, const float* w, const float* shift, const float* scale, int mod_ld, void* q,
                                   void* scales, float* rstd, int M, int D, int rows_per_batch, float eps, void* stream);
/* C[M,N] = dequant(Aq, As)[M,K] . dequant(Wq, Ws)[N,K]^T with the epilogues LDMAE_EPI_BIAS / LDMAE_EPI_GATE_RES / LDMAE_EPI_SWIGLU (and
 * LDMAE_EPI_TILE_LAUNCH or'ed in) exactly as the bf16 kernel writes them; out_dtype LDMAE_BF16 or LDMAE_F32 (SwiGLU: bf16).  lda / ldb are
 * the row strides of the element operands in bytes; the scale operands are dense [rows, K/32].  Covers M, N multiples of 8, K / lda / ldb
 * multiples of 128, element operands on 128-B lines, SwiGLU N % 256 == 0; the predicate says whether a shape is covered. */
int ldmae_gemm_nt_mx8_ok(int M, int N, int K, int lda, int ldb);
int ldmae_gemm_nt_mx8(int out_dtype, int epi, const void* Aq, const void* As, int lda, const void* Wq, const void* Ws, int ldb, void* C,
                      int ldc, int M, int N, int K, const float* bias, const float* xin, float* xout, const float* gate, int gate_ld,
                      int rows_per_batch, void* stream);
/* The qkv Linear with the QK-RMSNorm + RoPE epilogue of the bf16 kernel on the same operands (head dim 64; store_raw_qk = 0: only the v
 * third of qkv is written). */
int ldmae_gemm_nt_qkv_rope_mx8_ok(int B, int N, int H, int hd, int K, int lda, int ldb);
int ldmae_gemm_nt_qkv_rope_mx8(const void* Aq, const void* As, int lda, const void* Wq, const void* Ws, int ldb, const float* bias, void* qkv,
                               void* q2, void* k2, const float* wq, const float* wk, const float* cos, const float* sin, int B, int N,
                               int H, int hd, int K, float eps, int store_raw_qk, int tile_launch, void* stream);
/* Launch counts of this mode since the last reset, separate from the nine family slots above: counts[0] = quantise passes, counts[1] =
 * norm + quantise passes, counts[2] = block-scaled GEMMs.  n <= 3. */
#define LDMAE_MX8_COUNT_QUANTIZE 0
#define LDMAE_MX8_COUNT_NORM_QUANTIZE 1
#define LDMAE_MX8_COUNT_GEMM 2
int ldmae_mx8_launch_counts(long* counts, int n, int reset);

/* ---- Linear-probe and k-NN evaluation of tokenizer features (csrc/linprobe.hip, ldmae_amd/linear_probe.py) ----
 * No atomics: every sum has one fixed order, two launches on the same inputs give the same bits.  The entry points that take a dtype code
 * refuse every code they have no kernel for (the rule at the dtype codes above).
 * token_mean (f32, bf16, fp16 -> f32): out [B, D] = (1 / N) sum_n x[b, n, col0 + d]; token row (b, n) starts at x + (b N + n) ldx, so a
 *   channel slice of a wider token buffer is read in place.  f32 sums: 16 row groups of rows n = g, g + 16, ... in ascending order, the 16
 *   group sums in ascending order, one true division by N.
 * bn1d_fwd (f32): BatchNorm1d(affine = False).  training != 0: mean [D] = the f32 rounding of the column mean, var = the f32 rounding of
 *   sum (x - mean)^2 / B with THAT mean (two passes, never E[x^2] - mean^2; both sums in f64), xhat = (x - mean) * (1 / sqrtf(var + eps));
 *   run_mean = momentum mean + (1 - momentum) run_mean, run_var likewise with the unbiased variance (sum / (B - 1)), both in place;
 *   save_mean / save_rstd [D] optional.  B = 1 is refused (torch does).  training == 0: mean = run_mean, var = run_var, nothing is updated.
 * softmax_xent (f32): logits [B, C] with row stride ld, labels int64 [B].  loss [B] = m + log sum exp(l - m) - l[y] (m the row maximum);
 *   dlogits (optional, row stride ldd) = (softmax - onehot) * grad_scale; rank [B] = #{c : l[c] > l[y]} + #{c < y : l[c] == l[y]} --
 *   comparisons of the given f32 values only: top-1 is rank == 0, top-5 rank < 5.  Rows of C <= 4096 are read once and kept in registers.
 *   The caller checks labels against [0, C) on their host copy (ops.check_labels); a label outside gives loss NaN, rank -1, a zero gradient
 *   row and reads nothing.
 * lars_norms + lars_step (f32): the update of the reference's VMAE/util/lars.py.  lars_norms: norms [2] = (|p|, |g + wd p|) over n elements:
 *   squares and sums in f64, one partial pair per 4096 elements in the workspace (lars_workspace_bytes(n) bytes, 8-byte aligned), then one
 *   block adds the partials and stores the two square roots as f32.  lars_step: norms != NULL (a tensor of more than one dimension):
 *   dp = (g + wd p) * q, q = trust |p| / |dp| where both norms are positive, else 1; norms == NULL (a bias): dp = g; then mu = momentum mu +
 *   dp, p -= lr mu (each line one fma).  The step reads the norms from device memory: nothing comes back to the host.
 * topk_merge: sims [M, Nc] (row stride ld) are the similarities of M queries to bank rows col0 .. col0 + Nc - 1; vals / idx [M, k] are the
 *   running lists, sorted by value descending, then index ascending, empty slots (-inf, -1) last (the caller starts from all-empty
 *   lists).  After the call they hold the best k of the old list and the chunk.  Comparisons only: exact, whatever the chunking.  A NaN
 *   similarity is never taken.  k <= LDMAE_TOPK_MAX_K.
 * knn_vote: per query, score[c] = sum over the list's neighbours j (in list order) with bank_labels[idx_j] == c of exp(vals_j /
 *   temperature); rank [M] = the rank of qlabels[m] among the scores by softmax_xent's rule (ties to the lower class).  The scores of a query
 *   are held in LDS: C <= LDMAE_KNN_VOTE_MAX_C.  Empty slots, indices outside [0, nbank) and bank labels outside [0, C) add nothing; a query
 *   label outside [0, C) gives rank -1.  scores (optional) [M, C] receives the class scores. */
#define LDMAE_TOPK_MAX_K 256
#define LDMAE_KNN_VOTE_MAX_C 12288
int ldmae_token_mean(int dtype, const void* x, long ldx, int col0, float* out, int B, int N, int D, void* stream);
int ldmae_bn1d_fwd(int dtype, const void* x, int ldx, void* xhat, int ldo, float* run_mean, float* run_var, float* save_mean, float* save_rstd,
                   int B, int D, float eps, float momentum, int training, void* stream);
int ldmae_softmax_xent(int dtype, const void* logits, int ld, const long long* labels, float* loss, void* dlogits, int ldd, int* rank, int B,
                       int C, float grad_scale, void* stream);
long ldmae_lars_workspace_bytes(long n);
int ldmae_lars_norms(int dtype, const void* p, const void* g, long n, float wd, void* workspace, float* norms, void* stream);
int ldmae_lars_step(int dtype, void* p, const void* g, void* mu, long n, const float* norms, float lr, float wd, float momentum, float trust,
                    void* stream);
/* out [M, D] = x [M, D] / max(sqrtf(sqnorms[m]), 1e-12) (torch's F.normalize; sqnorms from ldmae_row_sqnorms_f32); out may be x. */
int ldmae_l2_normalize(const float* x, const float* sqnorms, float* out, long M, int D, void* stream);
int ldmae_topk_merge(const float* sims, int ld, int M, int Nc, int col0, float* vals, int* idx, int k, void* stream);
int ldmae_knn_vote(const float* vals, const int* idx, int M, int k, const long long* bank_labels, int nbank, const long long* qlabels, int C,
                   float temperature, int* rank, float* scores, void* stream);

/* ---- Held-out validation of the flow-matching objective (csrc/fm_valid.hip, ldmae_amd/validate.py) ----
 * f32, 16-byte accesses, no atomics, every sum in one fixed order.
 * fm_valid_plan: the model input xt and the regression target ut [B, C, HW] of a validation batch in one launch.  stored: [B, 2C, HW]
 *   (mean | logvar halves) when sample = 1, else the plain latents [B, C, HW]; idx [B] int64: the GLOBAL index of each sample; t [B]: its time;
 *   lat_mean / lat_std [C] or both NULL.  With n = C HW, z = the n values ldmae_normal_f32(., n, seed, 2 idx[b]) writes and x0 = those of
 *   counter 2 idx[b] + 1 (counters taken mod 2^64; z is drawn only when sample = 1):
 *     x1 = ldmae_latent_prologue's expression on (stored, z): ((mean + exp(0.5 clamp(logvar, -30, 20)) z) - lat_mean) / lat_std * multiplier
 *     xt = t x1 + (1 - t) x0: 1 - t rounded, each product rounded, then the sum rounded (no fma: ICPlan.plan operation by operation)
 *     ut = x1 - x0
 *   so the rows of sample i depend on (stored, seed, i, t) alone, whatever batch, position or rank they are computed in.  Neither draw is
 *   stored.  HW % 4 == 0; stored, xt, ut 16-byte aligned; xt and ut must not overlap.
 * row_mse: loss[b] = (sum_j (float(a[b, j]) - u[b, j])^2) / m for B dense rows of m elements, a f32 or bf16 (a_dtype), u f32: the difference
 *   rounded once, one fma chain per thread over its elements of a 4096-element chunk, the block sum of ldmae_rowdot_f32, partial[b ceil(m / 4096)
 *   + c], one block per row folds its chunks and divides by m (a true division).  4-element loads (16 bytes of f32, 8 of bf16) when every row
 *   start of a and u is aligned for them, element loads otherwise (another, equally fixed, order).  partial: ldmae_row_mse_partials(B, m)
 *   floats. */
int ldmae_fm_valid_plan_f32(const float* stored, const long long* idx, const float* t, const float* lat_mean, const float* lat_std,
                            float multiplier, int sample, unsigned long long seed, float* xt, float* ut, int B, int C, int HW, void* stream);
long ldmae_row_mse_partials(int B, long m);
int ldmae_row_mse(int a_dtype, const void* a, const float* u, float* loss, int B, long m, float* partial, void* stream);

/* ---- Guidance rules of the sampler (csrc/guidance.hip, ldmae_amd/guidance.py) ----
 * Time convention: x_t = t x1 + (1 - t) x0, the model predicts v = x1 - x0, the data prediction is x_t + (1 - t) v.
 * guidance_combine: pos (the main / conditional output p), neg (the null-class or guide-model output q) [B, C, HW] f32 or bf16 (in_dtype),
 *   out [B, C, HW] f32, one launch.  The first k channels (1 <= k <= C) of each sample, n_g = k HW contiguous elements, are guided; the sums
 *   below run over those n_g elements of ONE sample.  f32 arithmetic with every rounding as written (fma = one rounding), except the sums
 *   and the scalars derived from them, which are f64.  s = scale.
 *   LDMAE_GUIDE_CFG      g = fma(s, p - q, q).
 *   LDMAE_GUIDE_RESCALE  g0 = fma(s, p - q, q) (f32); std = the unbiased sample standard deviation (torch.std) of the f32 values p and g0, from
 *                        the f64 sums of (v - v_0) and (v - v_0)^2, v_0 the sample's first value (equal values: exactly 0); ratio = std(p) /
 *                        std(g0), or 1 when std(g0) == 0; f = (float)(1 + phi (ratio - 1)) [= phi ratio + 1 - phi]; g = g0 * f.  phi in [0, 1],
 *                        n_g >= 2.
 *   LDMAE_GUIDE_APG      omt = 1 - t[b]; d = p - q, then d = fma(momentum, m_prev, d) when momentum != 0 (m_prev = mom[b, i]); u = fma(omt, p, x);
 *                        <d, d>, <d, u>, <u, u> in f64; gamma = min(1, r / (omt sqrt<d, d>)) when r = norm_threshold > 0 and the denominator
 *                        is > 0, else 1; c = <d, u> / <u, u>, or 0 when <u, u> == 0; a = (float)((s - 1) gamma), b = (float)((1 - eta) c);
 *                        g = fma(a, fma(-b, u, d), p) [= p + (s - 1) gamma (d - (1 - eta) par), par = c u]; mom[b, i] = d when mom is given.
 *                        x [B, C, HW] f32 (the state), t [B] f32; mom NULL or [B, n_g] f32, updated in place; momentum != 0 needs it.
 *                        With eta = 1, r = 0, momentum = 0 it is cfg up to rounding.  x, t, mom are ignored by the other rules.
 *   Channels k .. C-1 of out are pos widened to f32, bit for bit.  out may be pos itself when pos is f32; it overlaps nothing else.
 *   Order: thread t of the sample's 1024 adds its 4-element groups t, t + 1024, ... in order, a wave joins its lanes in the xor butterfly
 *   32 .. 1, the 16 wave sums are added as a chain.  It depends on n_g alone: the rows of sample b depend on that sample's inputs only (alone
 *   or in a batch: same bits), two runs give the same bits, and so do the two access paths: 16-byte accesses (8 bytes of bf16) when
 *   HW % 4 == 0 and every pointer is 16-byte (bf16: 8-byte) aligned, element accesses otherwise.  No atomics, no workspace. */
#define LDMAE_GUIDE_CFG 0
#define LDMAE_GUIDE_RESCALE 1
#define LDMAE_GUIDE_APG 2
int ldmae_guidance_combine(int rule, int in_dtype, const void* pos, const void* neg, const float* x, const float* t, float* mom, float* out,
                           int B, int C, int HW, int k, float scale, float phi, float eta, float norm_threshold, float momentum, void* stream);

/* ---- Dispersive Loss on one block's features (csrc/dispersive.hip, transport.Transport(dispersive=...)) ----
 * Wang & He 2025, "Diffuse and Disperse: Image Generation with Representation Regularization", the InfoNCE-L2 variant.  z [B, K] f32 dense:
 * the f32 residual stream after one block, flattened per sample (K = N D); tau > 0.
 *     d_ij = ||z_i - z_j||^2                      (d_ii = 0)
 *     e_ij = exp(-d_ij / (K tau))     r_i = sum_j e_ij     S = sum_i r_i      (diagonal included: S >= B)
 *     L    = log S - 2 log B                      (= log mean_ij e_ij; B = 1: L = 0)
 *     dL/dz = C z,  C_ij = 4 / (S K tau) (e_ij - delta_ij r_i)                (C symmetric, rows sum to zero: sum_i dL/dz_i = 0)
 *   The largest exponent is 0, on the diagonal: no running maximum, no overflow.  When every off-diagonal e underflows, L = -log B and C = 0.
 * dispersive_fwd: loss [1] f32 and C [B, B] f32.  G = z z^T on v_mfma_f32_32x32x2_f32 with exact f32 operands, only the 64 x 64 tiles on or above
 *   the diagonal; K is cut into ldmae_dispersive_slabs(B, K) slabs, a block writes its partial tiles to the workspace and G is their sum in slab
 *   order.  Within a slab G_ij is one f32 fma chain over k, the same order for every (i, j).  Then, in f64: d_ij = max(G_ii + G_jj - 2 G_ij, 0),
 *   d_ii = 0 set, e = exp(-d / (K tau)) with K tau formed in f64 from the f32 tau; r_i: thread t of 256 adds j = t, t + 256, ... in order, then the
 *   fixed-order block sum; S likewise over r; L = (float) log(S / B^2); C_ij = (float)(4 / (S K tau) (e_ij - delta_ij r_i)), bitwise symmetric.
 *   No atomics: two calls give the same bits.  workspace: ldmae_dispersive_workspace_bytes(B, K) bytes, 16-byte aligned.
 * dispersive_bwd: dz [B, K] = g * (C z), g = upstream gradient times the weight, by value: one f32 fma chain over j per element (on the same
 *   MFMA, one writer per element), then one multiply by g.  dz overlaps neither input.
 * 1 <= B <= 1024, K % 4 == 0, z and dz 16-byte aligned. */
int ldmae_dispersive_slabs(int B, long K);
long ldmae_dispersive_workspace_bytes(int B, long K);
int ldmae_dispersive_fwd(const float* z, float* loss, float* C, int B, long K, float tau, void* workspace, void* stream);
int ldmae_dispersive_bwd(const float* C, const float* z, float g, float* dz, int B, long K, void* stream);

#ifdef __cplusplus
}
#endif
#endif

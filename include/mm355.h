/*
 * mm355.h -- C ABI of libmm355.so: the MI355X (gfx950 / CDNA4) kernels behind the MetaMorph hot path.
 *
 * The reference (facebookresearch/metamorph) has NO FFI layer: its boundary is the Python class
 * contract of metamorph.model and all device arithmetic is reached through torch /
 * transformers.  This header is therefore the ABI a maintainer would bind FROM the reference's Python
 * (ctypes); every entry point cites the reference call site whose arithmetic it
 * replaces.  Paths are relative to the reference checkout; "HF" = transformers (pinned 4.45.0 in
 * pyproject.toml:16, not vendored).
 *
 * Conventions
 *   - raw DEVICE pointers, caller allocates everything (no hipMalloc / hipFree / sync inside);
 *   - row-major, leading dimensions in ELEMENTS; bf16 is the storage type unless a name says f32;
 *   - 16-byte aligned base pointers and leading dimensions that are multiples of 8 elements;
 *   - asynchronous on `stream` (a hipStream_t passed as void*);
 *   - returns 0 or a negative MM355_E* code; never throws, never exits;
 *   - re-entrant; the only process-wide state is one-time kernel attribute setup (LDS size caps) -- no environment variable is read,
 *     nothing depends on the call sequence.
 */
#ifndef MM355_H
#define MM355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MM355_VERSION 100            /* 0.1.0 */

#define MM355_OK            0
#define MM355_EINVAL       -1        /* bad pointer / dimension / alignment                */
#define MM355_EUNSUPPORTED -2        /* legal request this build has no kernel for         */
#define MM355_ELAUNCH      -3        /* hipLaunch reported an error (hipGetLastError)      */

typedef uint16_t mm355_bf16;         /* raw bfloat16 bits                                  */

int mm355_version(void);
const char* mm355_strerror(int code);

/* ------------------------------------------------------------------------------------------------
 * GEMM family.   C[M,N] = epilogue( A[M,K] . B[N,K]^T )      (y = x W^T, the nn.Linear form)
 * Replaces every nn.Linear reached on the path: HF LlamaAttention/LlamaMLP projections
 * (metamorph_llama.py:349-359), lm_head (:398), mm_projector (multimodal_projector/builder.py:52-59),
 * vision_head (metamorph_llama.py:252-256), SigLIP q/k/v/out/fc1/fc2 (siglip_encoder.py:141) and the
 * patch-embedding Conv2d lowered to a GEMM.  Backward GEMMs (dX = dY W, dW = dY^T X) use the same
 * entry point on transposed operands (mm355_transpose_bf16).
 *   epilogue: v = acc; if BIAS v += bias[n]; if GELU_* v = gelu(v); if RESIDUAL v += R[m % res_mod][n];
 *             if ACCUMULATE v += C_old[m][n];  store as bf16 (or f32 with OUT_F32).
 * Requirements: K % 8 == 0, lda/ldb % 8 == 0 (ldc/ldr % 8 == 0 for bf16 vector stores, else scalar tail).
 * variant: 0 = auto (ping-pong 256x256 kernel, variant 11, once >= 200 tiles and K % 64 == 0; 128x128 LDS-DMA otherwise);
 *          for bench / tests: 1 = 128x128 register-staged (any K % 8 == 0), 2 = 128x128 LDS-DMA, 7 = 256x256 LDS-DMA software-pipelined,
 *          9 = 64x128 LDS-DMA, 11 = the 256x256 ping-pong kernel (falls back to 7 when K % 128 != 0 or an offset passes 2 GiB); 2, 7, 9 and 11
 *          need K % 64 == 0.  Any other number returns MM355_EUNSUPPORTED (mm355_gemm_num_variants() keeps the numbering of the
 *          retired ones).
 * ------------------------------------------------------------------------------------------------ */
#define MM355_GEMM_BIAS        1u
#define MM355_GEMM_GELU_ERF    2u    /* nn.GELU() default (projector, vision_head)         */
#define MM355_GEMM_GELU_TANH   4u    /* SigLIP "gelu_pytorch_tanh"                          */
#define MM355_GEMM_RESIDUAL    8u
#define MM355_GEMM_ACCUMULATE 16u
#define MM355_GEMM_OUT_F32    32u

int mm355_gemm_bf16(const mm355_bf16* A, int64_t lda, const mm355_bf16* B, int64_t ldb,
                    void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                    const mm355_bf16* bias, const mm355_bf16* residual, int64_t ldr, int64_t res_row_mod,
                    uint32_t flags, int variant, void* stream);
int mm355_gemm_num_variants(void);

/* Split-K form for PROMPT-PASS shapes (reference: the same nn.Linear calls, reached with a few hundred rows when `generate` runs the prompt,
 * metamorph_llama.py:665-717): C[M][N] = bf16(A . B^T (+ residual)) with K cut into slices that run as separate workgroups of ONE launch (64 x
 * 128 tiles x slices; fp32 partials in `workspace`, summed in slice order by a second launch).  At M <= ~1000 against N = 4096 .. 6144 the plain
 * kernels are a latency chain of one LDS-DMA round trip per K tile (down_proj, K = 14336: 184 us at any such M); the slices run side by side.
 * Not bit-identical to mm355_gemm_bf16 (another fp32 summation order).  workspace: mm355_gemm_splitk_ws_floats(M, N, K) floats (0: the shape
 * is not split -- the call then forwards to mm355_gemm_bf16 and needs none).  K % 64 == 0, N % 8 == 0, leading dimensions % 8 == 0. */
int64_t mm355_gemm_splitk_ws_floats(int64_t M, int64_t N, int64_t K);
int mm355_gemm_splitk_bf16(const mm355_bf16* A, int64_t lda, const mm355_bf16* B, int64_t ldb, mm355_bf16* C, int64_t ldc,
                           int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, float* workspace,
                           int64_t workspace_floats, void* stream);
/* The split projection with the launch that FOLLOWS it on the decode / prompt path folded into the reduce launch (a launch costs 3 - 5 us whatever
 * it does; the decode step of more than 16 sequences had thirteen per layer, nine with these).  Each form rounds the slice sums to bf16 where
 * mm355_gemm_splitk_bf16 stores them and continues with the arithmetic of the kernel it replaces: the bits of the launch sequence.  A shape that
 * is not split runs that sequence inside the library.  Reference: HF LlamaDecoderLayer at decode shape, metamorph_llama.py:665-717.
 *   _norm:        C[M][N] = bf16(A . B^T + residual) (rows N apart), Y[M][N] = RMSNorm(C; norm_w, eps)   == gemm_splitk -> rmsnorm_fwd
 *                 (o projection -> post-attention norm; down projection -> the next layer's input norm).  workspace: mm355_gemm_splitk_ws_floats.
 *   _swiglu:      act[M][I] = SiLU(g) * u, [g | u] = X . Wgu[2 I][K]^T                                    == gemm_splitk -> swiglu_fwd
 *                 workspace: mm355_gemm_splitk_swiglu_ws_floats(M, I, K) floats (never 0: the unsplit sequence parks its bf16 g | u rows there).
 *                 I % 4 == 0 where the problem is split (I % 8 != 0 or act rows without 16-byte alignment: the reduce launch writes one
 *                 output per thread, same arithmetic); the unsplit sequence keeps mm355_swiglu_fwd's I % 8 == 0.
 *   _rope_append: one new q|k|v row per sequence: q rotated at positions[m] (device) -> qkv[m][0 .. Hq d), rotated k and v -> cache row
 *                 positions[m]; the k | v columns of qkv are not written                                   == gemm_splitk -> rope_kv_append
 *                 workspace: mm355_gemm_splitk_ws_floats(M, (Hq + 2 Hkv) d, K).  M <= 65535, d % 16 == 0. */
int mm355_gemm_splitk_norm_bf16(const mm355_bf16* A, int64_t lda, const mm355_bf16* B, int64_t ldb, mm355_bf16* C, int64_t M, int64_t N,
                                int64_t K, const mm355_bf16* residual, int64_t ldr, const mm355_bf16* norm_w, float eps, mm355_bf16* Y,
                                float* workspace, int64_t workspace_floats, void* stream);
int64_t mm355_gemm_splitk_swiglu_ws_floats(int64_t M, int64_t I, int64_t K);
int mm355_gemm_splitk_swiglu_bf16(const mm355_bf16* X, int64_t ldx, const mm355_bf16* Wgu, int64_t ldw, mm355_bf16* act, int64_t ld_act,
                                  int64_t M, int64_t I, int64_t K, float* workspace, int64_t workspace_floats, void* stream);
int mm355_gemm_splitk_rope_append_bf16(const mm355_bf16* X, int64_t ldx, const mm355_bf16* Wqkv, int64_t ldw, mm355_bf16* qkv, int64_t ld_qkv,
                                       int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K, const mm355_bf16* cos_t,
                                       const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache, mm355_bf16* v_cache,
                                       int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats, void* stream);

/* Fused gate|up projection + SwiGLU of the LLaMA MLP (reference: HF LlamaMLP `down_proj(act_fn(gate_proj(x)) * up_proj(x))`, reached at
 * metamorph_llama.py:349-359):  gu[M][2 I] = X[M][K] . Wgu[2 I][K]^T  (gate columns 0..I-1, up columns I..2I-1, exactly what
 * mm355_gemm_bf16 writes) AND act[M][I] = bf16(silu(gate)) * up from the bf16-rounded gu values (exactly what mm355_swiglu_fwd writes), in
 * ONE launch: a workgroup's 256 tile columns are 128 gate channels and the same 128 up channels, so the product is formed in the epilogue
 * registers and the separate read of gu disappears.  Requirements: I % 128 == 0, K % 128 == 0, leading dimensions % 8 == 0;
 * MM355_EUNSUPPORTED otherwise (callers fall back to mm355_gemm_bf16 + mm355_swiglu_fwd: same bits). */
int mm355_gemm_swiglu_bf16(const mm355_bf16* X, int64_t ldx, const mm355_bf16* Wgu, int64_t ldw, mm355_bf16* gu, int64_t ld_gu,
                           mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, void* stream);

/* Fused q|k|v projection + RoPE (reference: HF LlamaAttention q_proj / k_proj / v_proj + apply_rotary_pos_emb, reached at
 * metamorph_llama.py:349-359), head size 128:  qkv[M][N] = X[M][K] . Wqkv[N][K]^T with the rotate-half rotation of mm355_rope_qk applied
 * in the epilogue to the columns below n_rot (= (Hq + Hkv) * 128: the q and k blocks; the v block is stored unrotated) -- the bits of
 * mm355_gemm_bf16 followed by mm355_rope_qk[_pos], without the in-place pass over q and k.  Row r is position r % L (+ pos_offset[r / L]
 * when pos_offset != NULL) of the cos / sin tables ([positions][128] bf16 from mm355_rope_table).  Requirements: N % 256 == 0,
 * n_rot % 128 == 0, K % 128 == 0, leading dimensions % 8 == 0; MM355_EUNSUPPORTED otherwise. */
int mm355_gemm_rope_bf16(const mm355_bf16* X, int64_t ldx, const mm355_bf16* Wqkv, int64_t ldw, mm355_bf16* qkv, int64_t ld_qkv,
                         const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* pos_offset,
                         int64_t M, int64_t N, int64_t K, int64_t L, int64_t n_rot, void* stream);

/* Fused backward of the same MLP stage: d act[M][I] = dY[M][K] . WdT[I][K]^T (the down_proj input gradient; WdT = down_proj.weight
 * transposed, [I][K]) is formed in the accumulators, rounded to bf16, and fed straight into the SwiGLU backward with gate / up from
 * gu[M][2 I]:  dgu[M][2 I] (row-major: the operand of the gate|up input-gradient GEMM) AND the contraction-major copies actT[I][ldT],
 * dguT[2 I][ldT] (the operands of the down_proj / gate|up weight-gradient GEMMs) -- the outputs of mm355_gemm_bf16 + mm355_swiglu_bwd_t,
 * without d act ever reaching memory.  Requirements: I % 64 == 0, M % 8 == 0, K % 128 == 0, ldT >= M, leading dimensions % 8 == 0;
 * MM355_EUNSUPPORTED otherwise.  Columns [M, ldT) of actT / dguT are not written (callers zero their padding). */
int mm355_gemm_swiglu_bwd_bf16(const mm355_bf16* dY, int64_t ldy, const mm355_bf16* WdT, int64_t ldw, const mm355_bf16* gu, int64_t ld_gu,
                               mm355_bf16* dgu, int64_t ld_dgu, mm355_bf16* actT, mm355_bf16* dguT, int64_t ldT,
                               int64_t M, int64_t I, int64_t K, void* stream);

/* Two independent problems of the form above, C0 (+)= A0 . B0^T and C1 (+)= A1 . B1^T, in ONE launch of the 256x256 ping-pong
 * kernel.  A launch runs in waves of 256 workgroups (one tile per CU): the LLaMA-3-8B weight gradients of qkv (384 tiles) and
 * down_proj (896 tiles) cost 2 + 4 wave times launched separately and 5 as a pair.  The host side pairs them at the end of
 * DecoderLayerFn.backward (reference: the two nn.Linear weight gradients autograd computes in LlamaDecoderLayer's backward,
 * call site metamorph_llama.py:349-359).
 * flags per problem: MM355_GEMM_ACCUMULATE, MM355_GEMM_OUT_F32.  Requirements per problem: K % 128 == 0, lda/ldb % 8 == 0,
 * 256 rows x ld x 2 B below 2 GiB (else MM355_EUNSUPPORTED: launch them one by one with mm355_gemm_bf16). */
int mm355_gemm_pair_bf16(const mm355_bf16* A0, int64_t lda0, const mm355_bf16* B0, int64_t ldb0, void* C0, int64_t ldc0,
                         int64_t M0, int64_t N0, int64_t K0, uint32_t flags0,
                         const mm355_bf16* A1, int64_t lda1, const mm355_bf16* B1, int64_t ldb1, void* C1, int64_t ldc1,
                         int64_t M1, int64_t N1, int64_t K1, uint32_t flags1, void* stream);

/* out[c][r] = in[r][c]   (rows x cols -> cols x rows), bf16.  Used for the backward GEMM operands.
 * ld_in % 8 == 0, in / out 16-byte aligned, ld_out >= rows (else MM355_EINVAL: output rows would overlap). */
int mm355_transpose_bf16(const mm355_bf16* in, int64_t ld_in, int64_t rows, int64_t cols,
                         mm355_bf16* out, int64_t ld_out, void* stream);

/* column sums: db[n] += sum_m dY[m][n]  (bias gradients of mm_projector / vision_head).  Deterministic: one workgroup owns 64 columns
 * and all M rows (four row phases, fixed-order reduction), no atomics. */
int mm355_colsum_bf16(const mm355_bf16* dY, int64_t ld, int64_t M, int64_t N, float* db_f32, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RMSNorm -- HF LlamaRMSNorm (fp32 normalise, cast to bf16, THEN multiply by weight); K7.
 * bwd: dx[m] = (dres ? dres[m] : 0) + d/dx ; dw_f32[h] += sum_m dy*xhat (caller zeroes dw_f32).
 * workspace (optional, mm355_rmsnorm_bwd_ws_floats(M, h) floats, 16-B aligned): the weight gradient is then summed
 * from per-workgroup partial rows in a fixed order (deterministic, no atomics); NULL = fp32 atomics on dw_f32.
 * ------------------------------------------------------------------------------------------------ */
int mm355_rmsnorm_fwd(const mm355_bf16* x, const mm355_bf16* w, mm355_bf16* y, int64_t M, int64_t h,
                      float eps, void* stream);
/* the same, also returning rstd[m] = rsqrt(mean(x[m]^2) + eps) (fp32, M values; NULL = not wanted) ... */
int mm355_rmsnorm_fwd_rstd(const mm355_bf16* x, const mm355_bf16* w, mm355_bf16* y, float* rstd_out, int64_t M, int64_t h,
                           float eps, void* stream);
/* ... from which the backward pass takes the TRANSPOSED normalised activations in one pass:
 *   out_t[c][m] = w[c] * bf16(x[m][c] * rstd[m]),   out_t is [h][ld_out], ld_out >= M (columns M..ld_out are not written)
 * = the contraction-major operand of the qkv / gate_up weight-gradient GEMMs (HF computes those from the saved norm output,
 * reference call site metamorph_llama.py:349-359); bit-identical to transposing mm355_rmsnorm_fwd's result. */
int mm355_rmsnorm_apply_t(const mm355_bf16* x, const mm355_bf16* w, const float* rstd, int64_t M, int64_t h,
                          mm355_bf16* out_t, int64_t ld_out, void* stream);
int mm355_rmsnorm_bwd(const mm355_bf16* dy, const mm355_bf16* x, const mm355_bf16* w,
                      const mm355_bf16* dres, mm355_bf16* dx, float* dw_f32, float* workspace,
                      int64_t M, int64_t h, float eps, void* stream);
int64_t mm355_rmsnorm_bwd_ws_floats(int64_t M, int64_t h);
/* the same with the weight gradient landing straight in the parameter's bf16 gradient buffer (training hot path: no fp32
 * scratch to zero, no separate accumulate pass): w_grad[h] = (accumulate ? w_grad : 0) + sum_m dy*xhat, fixed summation order;
 * workspace (mm355_rmsnorm_bwd_ws_floats floats) is required. */
int mm355_rmsnorm_bwd_wgrad(const mm355_bf16* dy, const mm355_bf16* x, const mm355_bf16* w, const mm355_bf16* dres,
                            mm355_bf16* dx, mm355_bf16* w_grad, int accumulate, float* workspace,
                            int64_t M, int64_t h, float eps, void* stream);

/* LayerNorm forward (SigLIP encoder, eps 1e-6); the tower is frozen in every shipped recipe. */
int mm355_layernorm_fwd(const mm355_bf16* x, const mm355_bf16* w, const mm355_bf16* b, mm355_bf16* y,
                        int64_t M, int64_t h, float eps, void* stream);
/* LayerNorm backward (trainable tower; HF SiglipEncoderLayer.layer_norm1/2 under freeze_vision=False,
 * siglip_encoder.py:138-141): dx = (dres ? dres : 0) + d/dx; dw_f32[h] += sum dy*xhat; db_f32[h] += sum dy, both summed in a
 * fixed order from per-workgroup partial rows in `workspace` (mm355_layernorm_bwd_ws_floats(M, h) floats, 16-B aligned). */
int64_t mm355_layernorm_bwd_ws_floats(int64_t M, int64_t h);
int mm355_layernorm_bwd(const mm355_bf16* dy, const mm355_bf16* x, const mm355_bf16* w, const mm355_bf16* dres,
                        mm355_bf16* dx, float* dw_f32, float* db_f32, float* workspace,
                        int64_t M, int64_t h, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RoPE -- HF apply_rotary_pos_emb, rotate-half convention, theta from config; K9.
 * Tables: cos/sin[L][d] bf16 (fp32 math, then cast -- LlamaRotaryEmbedding.forward).
 * mm355_rope_qk rotates the q and k column blocks of a fused qkv activation [B*L, ld] IN PLACE
 * (q heads at column 0, k heads at column Hq*d).  inverse != 0 applies the transposed rotation
 * (backward).  Position of row (b,l) is l.
 * ------------------------------------------------------------------------------------------------ */
int mm355_rope_table(mm355_bf16* cos_out, mm355_bf16* sin_out, int64_t L, int64_t d, float theta, void* stream);
/* Tables of a SCALED RoPE (config.rope_scaling / rope_parameters -- LLaMA-3.1's rope_type "llama3", "linear"; reference: MetaMorphConfig
 * inherits the field from LlamaConfig, metamorph_llama.py:129-133, and HF's LlamaRotaryEmbedding, reached at :349-359, rescales inv_freq
 * per wavelength band once at construction): inv_freq = float[d/2] on the DEVICE, computed by the caller exactly as
 * ROPE_INIT_FUNCTIONS[rope_type] does; table[l][j] = table[l][d/2 + j] = bf16(cos|sin(l * inv_freq[j]) * attention_scaling).  Every
 * consumer of the tables (mm355_rope_qk*, mm355_gemm_rope_bf16, the attention backward epilogues, the decode kernels) is unchanged. */
int mm355_rope_table_freq(mm355_bf16* cos_out, mm355_bf16* sin_out, int64_t L, int64_t d, const float* inv_freq, float attention_scaling,
                          void* stream);
int mm355_rope_qk(mm355_bf16* qkv, int64_t ld, int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d,
                  const mm355_bf16* cos_t, const mm355_bf16* sin_t, int inverse, void* stream);
/* the same with a per-sample position offset (int32[B], device): position of row (b,l) is l + pos_offset[b]; the tables need
 * L + max(pos_offset) rows.  Left-padded batches (tokenizer_padding_side = "left", metamorph_arch.py:362-386) are run right-aligned
 * to row 0 with pos_offset[b] = number of padding rows, which reproduces HF's position ids (arange(L), padding included). */
int mm355_rope_qk_pos(mm355_bf16* qkv, int64_t ld, int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d,
                      const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* pos_offset, int inverse, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention -- torch SDPA as driven by HF LlamaModel (causal + key padding, GQA, fp32 softmax; K10)
 * and by HF SiglipAttention (non causal, d = 72; K2).
 * q/k/v are column blocks of row-major activations: element (b,l,head,dd) at ptr[(b*L + l)*ld + head*d + dd]
 * (k and v share ld_k).  No transposed copies are needed: the kernels gather contraction-over-rows operands with
 * ds_read_b64_tr_b16.  seqlens[b] = number of valid (non padding) keys of sample b (right padding); NULL = L.
 * o: [B*L][>= Hq*d] bf16; lse: [B][Hq][L] f32 (natural-log sum-exp of the scaled scores).
 * Rows l >= seqlens[b] produce o = 0, lse = 0 (and zero gradients).
 * Supported d: any d % 8 == 0 and d <= 128 (64 / 128 LLaMA, 72 SigLIP SO400M).
 * ------------------------------------------------------------------------------------------------ */
int mm355_attn_fwd(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                   mm355_bf16* o, int64_t ld_o, float* lse, const int32_t* seqlens,
                   int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal, void* stream);

/* mm355_attn_fwd with the kernel generation chosen by the caller -- for tests and tools/ (A/B timing, the serialised debugging stream);
 * the product calls mm355_attn_fwd.  variant: 0 = as mm355_attn_fwd; 2 = the generic-d kernels; 4 = the one-wave-per-SIMD
 * hand-placed stream (d == 128); 41 = the same stream serialised (every LDS read waited for at once, 32 wait states behind every MFMA:
 * bit-identical to 4 by construction).  MM355_EUNSUPPORTED when the variant does not cover the geometry, and for variant 3 (a retired
 * kernel generation); MM355_EINVAL for any other number.  Same reference call site as
 * mm355_attn_fwd (torch SDPA reached at metamorph_llama.py:349-359). */
int mm355_attn_fwd_variant(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                           mm355_bf16* o, int64_t ld_o, float* lse, const int32_t* seqlens,
                           int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal, int variant, void* stream);

/* Diagnostics of the d == 128 stream (tests only; the product calls mm355_attn_fwd): mm355_attn_fwd_variant with variant 4 / 41 that also
 * reports how often each wave took the DEFERRED-RESCALE branch -- the kernel keeps a stale running row maximum m and rescales O and the
 * row sums only when some row of the wave's 64 query rows grew by more than 2^6 over it.  rescale_counts: int32 [B][Hq][ceil(L / 256)][4],
 * zeroed by the caller; entry = number of key tiles (of 64) at which that wave moved its maxima.  The parity tests on adversarial score
 * distributions (tests/test_attn_hostile_gpu.py) assert these counts against a CPU model of the kernel's decision rule, so that "the
 * branch ran" is a measured fact and not an assumption.  MM355_EUNSUPPORTED unless d == 128.  Same reference call site as mm355_attn_fwd
 * (torch SDPA reached at metamorph_llama.py:349-359). */
int mm355_attn_fwd_debug(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                         mm355_bf16* o, int64_t ld_o, float* lse, const int32_t* seqlens,
                         int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal, int variant,
                         int32_t* rescale_counts, void* stream);

/* delta[b][h][l] = sum_dd dO*O  (softmax-backward row term). */
int mm355_attn_bwd_prep(const mm355_bf16* o, const mm355_bf16* d_o, int64_t ld_o, float* delta,
                        int64_t B, int64_t L, int64_t Hq, int64_t d, void* stream);

/* Backward: dq / dk / dv are written as bf16 column blocks (leading dimensions ld_dq / ld_dkv), no atomics.
 * workspace: mm355_attn_bwd_ws_floats(...) floats; NULL allowed when that is 0 (d == 128 always needs it: MM355_EINVAL without).
 * The d == 128 kernels (LLaMA-3) sum a GQA group in registers (the dK/dV workgroup walks all query heads of its KV group) and use the
 * workspace only for 2*B*Hq*L per-row constants; the generic-d kernels under GQA (e.g. TinyLlama, d = 64) run one workgroup per
 * (KV tile, query head) and need 2*B*L*Hq*d floats for the per-head partials that are summed afterwards. */
int mm355_attn_bwd(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                   const mm355_bf16* d_o, int64_t ld_o, const float* lse, const float* delta, const int32_t* seqlens,
                   mm355_bf16* dq, int64_t ld_dq, mm355_bf16* dk, mm355_bf16* dv, int64_t ld_dkv,
                   int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal,
                   float* workspace, void* stream);

/* mm355_attn_bwd with the inverse RoPE rotation of dq / dk (what mm355_rope_qk(inverse = 1) does to the stored gradients: reference HF
 * apply_rotary_pos_emb backward, reached at metamorph_llama.py:349-359) applied in the kernels' epilogues: q and k are the POST-RoPE tensors the
 * forward attention saw, dq / dk come out as gradients of the PRE-RoPE projections.  Row l of sample b is position l (+ pos_offset[b]) of the
 * cos / sin tables ([positions][128] bf16).  d == 128 only (MM355_EUNSUPPORTED otherwise: call mm355_attn_bwd + mm355_rope_qk). */
int mm355_attn_bwd_rope(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                        const mm355_bf16* d_o, int64_t ld_o, const float* lse, const float* delta, const int32_t* seqlens,
                        mm355_bf16* dq, int64_t ld_dq, mm355_bf16* dk, mm355_bf16* dv, int64_t ld_dkv,
                        int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal,
                        const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* pos_offset, float* workspace, void* stream);

/* The general form: mm355_attn_bwd (cos_t = sin_t = NULL) or mm355_attn_bwd_rope (tables given) with the kernel generation chosen by the
 * caller: variant 0 = the product's choice; for tests / tools 2 = the generic-d kernels (under GQA their 2*B*L*Hq*d workspace is the
 * caller's to provide), 4 = the one-wave-per-SIMD hand-placed streams (d == 128, workspace required), 41 = the same streams serialised
 * (bit-identical to 4 by construction).  Variant 3 (a retired kernel generation) returns MM355_EUNSUPPORTED, any other number MM355_EINVAL.
 * Same reference call site as mm355_attn_bwd (backward of torch SDPA reached at metamorph_llama.py:349-359). */
int mm355_attn_bwd_variant(const mm355_bf16* q, const mm355_bf16* k, const mm355_bf16* v, int64_t ld_q, int64_t ld_k,
                           const mm355_bf16* d_o, int64_t ld_o, const float* lse, const float* delta, const int32_t* seqlens,
                           mm355_bf16* dq, int64_t ld_dq, mm355_bf16* dk, mm355_bf16* dv, int64_t ld_dkv,
                           int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, float scale, int causal,
                           const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* pos_offset,
                           float* workspace, int variant, void* stream);

/* floats of `workspace` mm355_attn_bwd needs for this geometry (ld_max = largest of ld_q / ld_k / ld_o); 0 when none is needed.
 * d == 128: 2 * B * Hq * L (the score chains' C operands -lse / scale and -delta); generic d under GQA: 2 * B * L * Hq * d. */
int64_t mm355_attn_bwd_ws_floats(int64_t B, int64_t L, int64_t Hq, int64_t Hkv, int64_t d, int64_t ld_max);

/* f32 [rows][cols] -> bf16 column block (generic helper). */
int mm355_cast_f32_bf16_2d(const float* in, int64_t ld_in, mm355_bf16* out, int64_t ld_out,
                           int64_t rows, int64_t cols, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Decode shape (greedy_decode / generate with a KV cache; reference metamorph_llama.py:502-597, which
 * re-runs the prefix every step).  HBM-bound streaming kernels.
 *   gemv: y[M,N] = x[M,K] . W[N,K]^T for M <= 16 new rows -- and for 17 .. 32 rows on WIDE weights (more than 1280 groups of 16 weight rows, i.e.
 *         N > 20480 for gemv, I > 10240 for gemv_swiglu without norm_w: gate|up, lm_head), where a second group of 16 x rows rides on the same
 *         weight fragments -- else MM355_EUNSUPPORTED: use mm355_gemm_bf16 / mm355_gemm_splitk_bf16.  Up to four rows run on the
 *         vector ALU with the x rows parked in LDS (windows of 4096 columns), so that only weight loads sit in the in-order
 *         vector-memory queue: one or two rows as an fp32 fma chain, three and four on v_dot2c_f32_bf16; 5 .. 16 rows on
 *         v_mfma_f32_16x16x32_bf16, the weight rows loaded coalesced and re-laid out into fragments through wave-private LDS.  flags
 *         BIAS / GELU_ERF / GELU_TANH / RESIDUAL / OUT_F32 as for the GEMM.  The weight is addressed with 32-bit byte offsets:
 *         N * ldw * 2 < 3.75 GiB (else the plain stream of mm355_gemv_bf16 for up to four rows; MM355_EUNSUPPORTED for more rows and for
 *         the fused forms below).
 *   attn_decode: one query row per (sample, head), q [B][Hq*d] (ld_q), caches [B][max rows][Hkv*d] (row stride ld_kv,
 *         sample stride batch_stride_kv), kv_lens[B] (device) valid cached rows INCLUDING the current one, max_kv_len an
 *         upper bound of them (sizes the launch and the workspace of mm355_attn_decode_ws_floats floats); GQA groups 1/2/4/8.
 *         ONE launch: the key group that finishes last merges the partials of its heads; the arrival counters are the FIRST B*Hq
 *         words of the workspace (whatever max_kv_len) -- zero them once before the first call (hipMemset), every call leaves them zero.
 *   gemv_swiglu: act[M][I] = SiLU(g) * u with [g | u] = n . Wgu[2I][K]^T formed in the GEMV's epilogue (g, u rounded to bf16 first:
 *         the bits of mm355_gemv_bf16 + mm355_swiglu_fwd); norm_w != NULL: n = RMSNorm(x; norm_w, eps) formed per workgroup on the
 *         fly (the bits of mm355_rmsnorm_fwd), else n = x.  HF LlamaMLP / LlamaRMSNorm at decode shape (metamorph_llama.py:502-597).
 *         With norm_w and 5 .. 16 rows all normalised rows stay in LDS: M * (K rounded up to 32 + 8) * 2 bytes <= 140 KiB, else MM355_EUNSUPPORTED
 *         (run mm355_rmsnorm_fwd first); up to four rows any K (windows of 4096 columns).  The same holds for gemv_rope_append.
 *   gemv_rope_append: the fused q|k|v projection of M new rows with RoPE at positions[m] (device) and the KV-cache append in the
 *         epilogue: q -> qkv[m][0 .. Hq*d), rotated k and v -> cache row positions[m] (the bits of mm355_gemv_bf16 +
 *         mm355_rope_kv_append); the k | v columns of `qkv` are not written.  norm_w as above.
 * ------------------------------------------------------------------------------------------------ */
int mm355_gemv_bf16(const mm355_bf16* x, int64_t ldx, const mm355_bf16* W, int64_t ldw, void* y, int64_t ldy,
                    int64_t M, int64_t N, int64_t K, const mm355_bf16* bias, const mm355_bf16* residual, int64_t ldr,
                    uint32_t flags, void* stream);
 /* rope_kv_append: one new fused qkv row per sample [B][(Hq+2Hkv)*d]: q and k rotated at positions[b] (device), q left in
 *         place, rotated k and v written to cache row positions[b] (graph-replayable: no host-side position). */
int mm355_rope_kv_append(mm355_bf16* qkv, int64_t ld, int64_t B, int64_t Hq, int64_t Hkv, int64_t d,
                         const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions,
                         mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, void* stream);
int mm355_gemv_swiglu_bf16(const mm355_bf16* x, int64_t ldx, const mm355_bf16* Wgu, int64_t ldw, mm355_bf16* act, int64_t ld_act,
                           int64_t M, int64_t I, int64_t K, const mm355_bf16* norm_w, float eps, void* stream);
int mm355_gemv_rope_append_bf16(const mm355_bf16* x, int64_t ldx, const mm355_bf16* Wqkv, int64_t ldw, mm355_bf16* qkv, int64_t ld_qkv,
                                int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K, const mm355_bf16* norm_w, float eps,
                                const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache,
                                mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, void* stream);
int64_t mm355_attn_decode_ws_floats(int64_t B, int64_t Hq, int64_t d, int64_t max_kv_len);
int mm355_attn_decode(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache,
                      int64_t ld_kv, int64_t batch_stride_kv, const int32_t* kv_lens, int64_t max_kv_len,
                      mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                      float* workspace, void* stream);
/* tests / tools: variant 0 = as mm355_attn_decode (one 1024-thread workgroup per sample, KV head and 1024 cached rows; the lone
 * workgroup of a cache of <= 1024 rows writes the output itself: no device-scope fence -- and, when max_kv_len <= 1024, the GQA group is
 * spread over one workgroup per query head (pairs of heads from 64 workgroups on): same arithmetic, bit-identical output, half the
 * launch time), 1 = one 256-thread workgroup per 256-row chunk + merge by the last, 2 = variant 0 with the whole GQA group in one
 * workgroup whatever the bound.  max_kv_len is a LAUNCH parameter: a caller that knows its lengths on the host passes 1024 while every
 * kv_lens[b] <= 1024 and the capacity afterwards (metamorph_amd.functional.decode_kv_bound). */
int mm355_attn_decode_variant(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache,
                      int64_t ld_kv, int64_t batch_stride_kv, const int32_t* kv_lens, int64_t max_kv_len,
                      mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                      float* workspace, int variant, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The decode GEMVs over weight-only FP8 (the reference serves its LLM in 8 bits through bitsandbytes: metamorph/model/builder.py:13-25,
 * load_pretrained_model(..., load_8bit=True); this is a scheme of its own, not LLM.int8).  fmt MM355_W8_E4M3: W[N][K] stored as OCP e4m3fn
 * bytes Wq[N][K] (the gfx950 encoding, not fnuz; row stride ldw_bytes), plus scale[N] fp32; dequantised value fp32(Wq[n][k]) * scale[n].
 *   gemv_w8: y[m][n] = epilogue(scale[n] * sum_k fp32(Wq[n][k]) * fp32(x[m][k])), x bf16, fp32 accumulation, the scale applied once, after
 *         the sum; flags and epilogue as mm355_gemv_bf16.  M <= 16 rows (more: MM355_EUNSUPPORTED -- mm355_gemm_w8 below).  Up to
 *         four rows on the vector ALU (v_cvt_pk_f32_fp8 + v_perm_b32 widen a pair of weights to packed bf16 for v_dot2c_f32_bf16), 5 .. 16 on
 *         v_mfma_f32_16x16x32_bf16 with the bytes widened in registers; x rows parked in LDS windows, a register ring of weight loads.
 *         fmt other than MM355_W8_E4M3, K % 16 != 0, ldw_bytes % 16 != 0, a NULL scale or misaligned pointers: MM355_EINVAL before any
 *         launch.  32-bit byte offsets: N * ldw_bytes < 3.75 GiB, else MM355_EUNSUPPORTED.
 *   gemv_swiglu_w8 / gemv_rope_append_w8: the twins of mm355_gemv_swiglu_bf16 / mm355_gemv_rope_append_bf16 (same row limits, same
 *         MM355_EUNSUPPORTED cases: odd I, d % 4 != 0, norm_w with 5 .. 16 rows beyond 140 KiB of rows): the bits of mm355_gemv_w8 +
 *         mm355_swiglu_fwd, of mm355_gemv_w8 + mm355_rope_kv_append, and with norm_w of mm355_rmsnorm_fwd in front.
 *   dequant_w8_bf16: out[n][k] = bf16(fp32(Wq[n][k]) * scale[n]) (RNE), a plain streaming kernel: the routes mm355_gemm_w8* do not take (passes of
 *         more than 4096 rows, projections that are not split) run the bf16 GEMMs on weights dequantised into a scratch buffer.  ld_out % 8 == 0, out 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
#define MM355_W8_E4M3 1
int mm355_gemv_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, void* y, int64_t ldy,
                  int64_t M, int64_t N, int64_t K, const mm355_bf16* bias, const mm355_bf16* residual, int64_t ldr,
                  uint32_t flags, void* stream);
int mm355_gemv_swiglu_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                         mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, const mm355_bf16* norm_w, float eps, void* stream);
int mm355_gemv_rope_append_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                              mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                              const mm355_bf16* norm_w, float eps, const mm355_bf16* cos_t, const mm355_bf16* sin_t,
                              const int32_t* positions, mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv,
                              int64_t batch_stride_kv, void* stream);
int mm355_dequant_w8_bf16(const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, mm355_bf16* out, int64_t ld_out,
                          int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The decode GEMVs over weight-only MXFP4 (the reference's other quantised mode: metamorph/model/builder.py:13-25, load_4bit=True; OCP MX,
 * not bitsandbytes' NF4).  fmt MM355_W4_MXFP4, K % 32 == 0: W[N][K] stored as e2m1 nibbles Wq[N][K/2] (row stride ldw_bytes; byte j of a
 * row holds k = 2j in bits 3:0 and k = 2j+1 in bits 7:4, the torch.float4_e2m1fn_x2 order; a nibble = sign (bit 3) + a code for |v| in
 * {0, 0.5, 1, 1.5, 2, 3, 4, 6}) plus one e8m0 scale byte per 32 consecutive k, S[N][K/32] (row stride lds_bytes): dequantised value
 * Wd[n][k] = e2m1(nibble) * 2^(S[n][k/32] - 127), exactly a bf16 value for S in 2 .. 252 (what ops.quantize_w4 emits; never 0xFF).
 * 4.25 bits per weight.  Coarser than FP8 (relative RMS weight error 0.114 against 0.026 on Gaussian weights): opt-in.
 *   gemv_w4: y[m][n] = epilogue(sum_k fp32(Wd[n][k]) * fp32(x[m][k])), x bf16, fp32 accumulation, the group scale inside the widening
 *         conversion (v_cvt_scalef32_pk_bf16_fp4: a byte and its scale -> a packed bf16 pair), nothing multiplied after the sum; flags
 *         and epilogue as mm355_gemv_bf16.  M <= 16 rows (more: MM355_EUNSUPPORTED -- mm355_gemm_w4 below).  Up to four
 *         rows on v_dot2c_f32_bf16, 5 .. 16 on v_mfma_f32_16x16x32_bf16; a 16-byte load is one scale group.  fmt other than
 *         MM355_W4_MXFP4, K % 32 != 0, ldw_bytes % 16 != 0, lds_bytes < K / 32, a NULL S or misaligned pointers: MM355_EINVAL before any
 *         launch.  32-bit byte offsets: N * ldw_bytes < 3.75 GiB, else MM355_EUNSUPPORTED.
 *   gemv_swiglu_w4 / gemv_rope_append_w4: the twins of mm355_gemv_swiglu_w8 / mm355_gemv_rope_append_w8 (S, lds_bytes in place of scale;
 *         same row limits and MM355_EUNSUPPORTED cases): the bits of mm355_gemv_w4 + mm355_swiglu_fwd, of mm355_gemv_w4 +
 *         mm355_rope_kv_append, and with norm_w of mm355_rmsnorm_fwd in front.
 *   dequant_w4_bf16: out[n][k] = bf16(Wd[n][k]), exact (no rounding), a plain streaming kernel: the routes mm355_gemm_w4* do not take
 *         (passes of more than 4096 rows, shapes the split-K GEMM does not split).  ld_out % 8 == 0, out 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
#define MM355_W4_MXFP4 2
int mm355_gemv_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                  void* y, int64_t ldy, int64_t M, int64_t N, int64_t K, const mm355_bf16* bias, const mm355_bf16* residual, int64_t ldr,
                  uint32_t flags, void* stream);
int mm355_gemv_swiglu_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                         mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, const mm355_bf16* norm_w, float eps, void* stream);
int mm355_gemv_rope_append_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                              int fmt, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                              const mm355_bf16* norm_w, float eps, const mm355_bf16* cos_t, const mm355_bf16* sin_t,
                              const int32_t* positions, mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv,
                              int64_t batch_stride_kv, void* stream);
int mm355_dequant_w4_bf16(const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt, mm355_bf16* out, int64_t ld_out,
                          int64_t N, int64_t K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The split-K GEMM over the same weight-only FP8 format: the prompt pass and decode steps of MORE than 16 sequences of a quantised decoder
 * stream the weight as bytes instead of dequantising it into a scratch buffer first (reference: the nn.Linear calls of the 8-bit model,
 * metamorph/model/builder.py:13-25 with metamorph_llama.py:665-717).  x[M][K] bf16, Wq[N][K] e4m3fn bytes (row stride ldw_bytes), scale[N] fp32.
 *   gemm_w8:  C[M][N] = scale[n] * sum_k fp32(Wq[n][k]) * fp32(x[m][k]) (+ residual), the twin of mm355_gemm_splitk_bf16: the SAME K slices
 *         (mm355_gemm_w8_ws_floats == mm355_gemm_splitk_ws_floats), the same 64-wide K tiles and MFMA order, the bytes widened to bf16 in
 *         registers (exact), so only the weight's storage differs.  The scale multiplies every fp32 partial where the GEMM launch stores it,
 *         and the reduce launch of the bf16 form adds the slices: C = bf16(sum_s scale[n] * P_s (+ residual)) -- for power-of-two scales the
 *         bits of mm355_gemm_splitk_bf16 on the dequantised weight, otherwise one fp32 rounding per slice away from scale[n] * sum_s P_s.
 *         flags: MM355_GEMM_RESIDUAL | MM355_GEMM_OUT_F32.  A shape that is not split (workspace 0: e.g. the lm_head) and every fp32 output
 *         run the same kernel as ONE slice that stores epilogue(scale[n] * P) straight into C; workspace may then be NULL.
 *   gemm_w8_norm / gemm_w8_swiglu / gemm_w8_rope_append: the twins of mm355_gemm_splitk_norm_bf16 / _swiglu_bf16 / _rope_append_bf16 (same
 *         operands, limits and workspaces; mm355_gemm_w8_swiglu_ws_floats == mm355_gemm_splitk_swiglu_ws_floats), the reduce launches shared
 *         with them; a shape that is not split runs gemm_w8 + mm355_rmsnorm_fwd / mm355_swiglu_fwd / mm355_rope_kv_append inside the library.
 *   Before any launch: fmt other than MM355_W8_E4M3, K % 64 != 0, ldw_bytes % 16 != 0, ldx % 8 != 0, a NULL scale, misaligned pointers or a
 *   workspace that is too small: MM355_EINVAL.  M > 4096: MM355_EUNSUPPORTED (larger passes: mm355_dequant_w8_bf16 + the bf16 GEMMs).
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_gemm_w8_ws_floats(int64_t M, int64_t N, int64_t K);
int mm355_gemm_w8(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, void* C, int64_t ldc,
                  int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags, float* workspace,
                  int64_t workspace_floats, void* stream);
int mm355_gemm_w8_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, mm355_bf16* C,
                       int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, const mm355_bf16* norm_w, float eps,
                       mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream);
int64_t mm355_gemm_w8_swiglu_ws_floats(int64_t M, int64_t I, int64_t K);
int mm355_gemm_w8_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt, mm355_bf16* act,
                         int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace, int64_t workspace_floats, void* stream);
int mm355_gemm_w8_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const float* scale, int fmt,
                              mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                              const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache,
                              mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * The split-K GEMM over the weight-only MXFP4 format (csrc/gemm_w4.hip): the prompt pass and decode steps of MORE than 16 sequences of a 4-bit
 * decoder stream the weight as nibbles instead of dequantising it into a scratch buffer first.  Operands as mm355_gemv_w4: x[M][K] bf16,
 * Wq[N][K/2] e2m1 nibbles (row stride ldw_bytes), S[N][K/32] e8m0 scale bytes (row stride lds_bytes), fmt MM355_W4_MXFP4.
 *   gemm_w4:  C[M][N] = sum_k fp32(Wd[n][k]) * fp32(x[m][k]) (+ residual), the twin of mm355_gemm_splitk_bf16 and mm355_gemm_w8: the SAME K
 *         slices (mm355_gemm_w4_ws_floats == mm355_gemm_splitk_ws_floats), the same 64-wide K tiles and MFMA order, the nibbles widened to
 *         bf16 in registers with the group scale inside the conversion (v_cvt_scalef32_pk_bf16_fp4, exact).  Nothing is multiplied after the
 *         sum and the partials of a split problem are plain, so for ANY scales the result is bit for bit that of mm355_gemm_splitk_bf16 on
 *         the output of mm355_dequant_w4_bf16.  flags: MM355_GEMM_RESIDUAL | MM355_GEMM_OUT_F32.  A shape that is not split (workspace 0)
 *         and every fp32 output run the same kernel as ONE slice that stores straight into C; workspace may then be NULL.
 *   gemm_w4_norm / gemm_w4_swiglu / gemm_w4_rope_append: the twins of mm355_gemm_w8_norm / _swiglu / _rope_append (S, lds_bytes in place of
 *         scale; same operands, limits and workspaces; mm355_gemm_w4_swiglu_ws_floats == mm355_gemm_splitk_swiglu_ws_floats), the reduce
 *         launches shared with the bf16 forms; a shape that is not split runs gemm_w4 + mm355_rmsnorm_fwd / mm355_swiglu_fwd /
 *         mm355_rope_kv_append inside the library.
 *   Before any launch: fmt other than MM355_W4_MXFP4, K % 64 != 0, ldw_bytes % 16 != 0, ldw_bytes < K / 2, lds_bytes < K / 32, ldx % 8 != 0,
 *   a NULL S, misaligned pointers or a workspace that is too small: MM355_EINVAL.  M > 4096: MM355_EUNSUPPORTED (larger passes:
 *   mm355_dequant_w4_bf16 + the bf16 GEMMs).  The kernel addresses Wq and S with 64-bit offsets: no limit on N * ldw_bytes.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_gemm_w4_ws_floats(int64_t M, int64_t N, int64_t K);
int mm355_gemm_w4(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt, void* C,
                  int64_t ldc, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, uint32_t flags, float* workspace,
                  int64_t workspace_floats, void* stream);
int mm355_gemm_w4_norm(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                       mm355_bf16* C, int64_t M, int64_t N, int64_t K, const mm355_bf16* residual, int64_t ldr, const mm355_bf16* norm_w,
                       float eps, mm355_bf16* Y, float* workspace, int64_t workspace_floats, void* stream);
int64_t mm355_gemm_w4_swiglu_ws_floats(int64_t M, int64_t I, int64_t K);
int mm355_gemm_w4_swiglu(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes, int fmt,
                         mm355_bf16* act, int64_t ld_act, int64_t M, int64_t I, int64_t K, float* workspace, int64_t workspace_floats,
                         void* stream);
int mm355_gemm_w4_rope_append(const mm355_bf16* x, int64_t ldx, const uint8_t* Wq, int64_t ldw_bytes, const uint8_t* S, int64_t lds_bytes,
                              int fmt, mm355_bf16* qkv, int64_t ld_qkv, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, int64_t K,
                              const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions, mm355_bf16* k_cache,
                              mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, float* workspace, int64_t workspace_floats,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cached decode over an FP8 KV cache (writing it: csrc/decode_kv8.hip; attention over it: csrc/attn_decode.hip).  fmt MM355_KV8_E4M3: one
 * cached head-row -- the d post-RoPE bf16 values of one KV head of one token -- is d OCP e4m3fn bytes plus ONE fp32 scale: scale = the
 * smallest power of two with amax / scale <= 448 (a row of zeros: 1), q[c] = RNE_e4m3(x[c] / scale) (exact shift, nothing saturates,
 * subnormals rounded, -0 kept; non-finite inputs are outside the contract).  fp32(q[c]) * scale is exact and a bf16 value, so every
 * reader equals the bf16 kernels on the dequantised rows bit for bit.
 * Bytes: [.., rows, Hkv * d] with row stride ld_*_bytes; scales: [.., rows, Hkv] fp32 with row stride ld_scale (floats); the batch strides
 * separate the sequences.
 *   kv_quant_f8: n_rows already-rotated bf16 rows src[r][Hkv * d] (row stride ld_src elements: e.g. the k columns of a fused q|k|v
 *         activation) -> cache row row0 + r % rows_per_seq of sequence r / rows_per_seq.  One head-row per 16-lane group.
 *   rope_kv_append_f8: the twin of mm355_rope_kv_append (device positions, graph-replayable): q rotated in place with the same bits, the
 *         rotated k rounded to bf16 as that kernel stores it and then quantised, v quantised; bytes and scales into cache row positions[b].
 *   attn_decode_f8(_variant): the kernel of mm355_attn_decode(_variant) instantiated for e4m3 rows, variants 0 and 2:
 *         s_j = k_scale[j] * sum_c fp32(K8[j][c]) * (fp32(q[c]) * scale), o[c] = sum_j (p_j * v_scale[j]) * fp32(V8[j][c]) / l -- each
 *         scale once per key, the sums in the order of the bf16 form (8 consecutive columns per lane, one 8-byte load), the same workspace
 *         (mm355_attn_decode_ws_floats), the same max_kv_len launch parameter and counter reset.  Equal to mm355_attn_decode on the
 *         dequantised cache, barring fp32 underflow.
 *   Before any launch: fmt other than MM355_KV8_E4M3, a NULL scale pointer, pointers or strides that are not 8-byte (src / qkv: 16-byte)
 *   aligned: MM355_EINVAL; d % 8 != 0 or d > 128: MM355_EUNSUPPORTED (rope_kv_append_f8 needs d % 16 == 0 as its twin does).
 * ------------------------------------------------------------------------------------------------ */
#define MM355_KV8_E4M3 1
int mm355_kv_quant_f8(const mm355_bf16* src, int64_t ld_src, int64_t n_rows, int64_t rows_per_seq, int64_t Hkv, int64_t d,
                      uint8_t* dst_bytes, int64_t ld_dst_bytes, float* dst_scale, int64_t ld_scale, int64_t batch_stride_bytes,
                      int64_t batch_stride_scale, int64_t row0, int fmt, void* stream);
int mm355_rope_kv_append_f8(mm355_bf16* qkv, int64_t ld, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, const mm355_bf16* cos_t,
                            const mm355_bf16* sin_t, const int32_t* positions, uint8_t* k_cache, uint8_t* v_cache, int64_t ld_kv_bytes,
                            int64_t batch_stride_kv_bytes, float* k_scale, float* v_scale, int64_t ld_scale, int64_t batch_stride_scale,
                            int fmt, void* stream);
int mm355_attn_decode_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                         int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                         int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                         int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, void* stream);
int mm355_attn_decode_f8_variant(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                 int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                 int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o,
                                 int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Extending a filled KV cache by n rows per sequence in one pass (csrc/attn_extend.hip): the shape between the prompt pass (mm355_attn_fwd: one
 * length for queries and keys) and the decode step (mm355_attn_decode: one query row per sequence) -- a follow-up turn of a conversation, a
 * prompt run in chunks, several candidate tokens scored against one cache (reference: the cached generate() of metamorph_llama.py:502-597).
 *   attn_extend: q [B*n][Hq*d] (ld_q), ALREADY rotated, row (b, i) at b * n + i; caches [B][rows][Hkv*d] as mm355_attn_decode takes them (row
 *         stride ld_kv, sequence stride batch_stride_kv); past[B] int32 on the device; o [B*n][Hq*d] (ld_o).  The cache already holds the
 *         chunk's own rows at past[b] .. past[b] + n - 1 (the append comes first); row (b, i) attends the keys j <= past[b] + i: o = softmax(
 *         scale * q K^T) V with the softmax in fp32 and the scale applied on the fp32 side.  max_kv_len is a host bound, past[b] + n <=
 *         max_kv_len <= rows: it sizes the launch and the workspace (mm355_attn_extend_ws_floats floats, 16-byte aligned; 0: workspace may be
 *         NULL) and no row >= max_kv_len is read whatever past[] says; cache rows >= past[b] + n are never read.  Right for n == 1 and
 *         past[b] == 0.  v_mfma_f32_16x16x32_bf16, K / V tiles through LDS, the query rows of a GQA group packed into one row tile so that a
 *         tile of the cache is read once per KV head; few workgroups (small n, long prefix): the key tiles are dealt to several workgroups
 *         and a second launch merges their partials.  The split is a function of (B, n, Hq, Hkv, max_kv_len) alone.
 *   attn_extend_f8: the same over an e4m3 cache (bytes and scales as mm355_attn_decode_f8 takes them): the bytes times the power-of-two scale
 *         are widened to bf16 on the way into LDS (exact, see above), the rest is the same code: equal to mm355_attn_extend on the dequantised
 *         cache bit for bit.
 *   Before any launch: fmt other than MM355_KV8_E4M3, a NULL pointer or scale, n > max_kv_len, Hq % Hkv != 0, q / o not 16-byte aligned or
 *   ld_q / ld_o % 8 != 0, cache pointers or strides not 16-byte (e4m3: 8-byte) aligned, a row stride shorter than a row, a workspace that is
 *   missing or too small: MM355_EINVAL; d % 8 != 0, d > 128 or a GQA group other than 1, 2, 4, 8: MM355_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_attn_extend_ws_floats(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t max_kv_len);
int mm355_attn_extend(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                      int64_t batch_stride_kv, const int32_t* past, int64_t n, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                      int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);
int mm355_attn_extend_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                         int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                         int64_t batch_stride_scale, int fmt, const int32_t* past, int64_t n, int64_t max_kv_len, mm355_bf16* o,
                         int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace,
                         int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Extending B filled (or empty) caches by DIFFERENT numbers of rows in one pass (csrc/attn_extend.hip): a ragged batch of prompts, or of
 * follow-up turns, as one packed row block (reference: the cached generate() of metamorph_llama.py:502-597, run per sequence).
 *   attn_extend_ragged: mm355_attn_extend with a row table in place of n.  row_start int32 [B + 1] on the device, non-decreasing: sequence b
 *         brings n_b = row_start[b + 1] - row_start[b] query rows, at rows row_start[b] + i of q / o [q_rows][Hq*d] (packed, no padding rows).
 *         The cache already holds them at past[b] .. past[b] + n_b - 1 of block b (the append comes first); row (b, i) attends the keys j <=
 *         past[b] + i of block b; fp32 softmax, the scale on the fp32 side.  Right for n_b == 0 (nothing of that sequence is read or written,
 *         its block included) and past[b] == 0 (a prompt).  n_max (host, >= every n_b) sizes the launch, the workspace
 *         (mm355_attn_extend_ragged_ws_floats) and the split: they are mm355_attn_extend's for n = n_max, a function of (B, n_max, Hq, Hkv,
 *         max_kv_len) alone, so with row_start[b] = b * n and n_max = n the output is mm355_attn_extend's bit for bit.  Workgroups whose row
 *         tile lies beyond n_b * G leave at once, and the merge launch skips the same rows.  A wrong table stays inside the buffers: n_b is
 *         clamped into [0, n_max], a row index into [0, q_rows), key rows below min(past[b] + n_b, max_kv_len); cache rows >= past[b] + n_b
 *         are never read and o rows that belong to no sequence are never written.
 *   attn_extend_ragged_f8: the same over an e4m3 cache; differs in the tile mover only: equal to the bf16 form on the dequantised cache bit
 *         for bit.
 *   Before any launch: mm355_attn_extend's refusals and codes (with n_max for n); a NULL row_start, n_max < 1, n_max > max_kv_len or q_rows < 1:
 *   MM355_EINVAL.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_attn_extend_ragged_ws_floats(int64_t B, int64_t n_max, int64_t Hq, int64_t Hkv, int64_t d, int64_t max_kv_len);
int mm355_attn_extend_ragged(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                             int64_t batch_stride_kv, const int32_t* past, const int32_t* row_start, int64_t n_max, int64_t q_rows,
                             int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                             float* workspace, int64_t workspace_floats, void* stream);
int mm355_attn_extend_ragged_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                int64_t batch_stride_scale, int fmt, const int32_t* past, const int32_t* row_start, int64_t n_max,
                                int64_t q_rows, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv,
                                int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * RoPE + cache append with a block and a position PER ROW (csrc/decode.hip, csrc/decode_kv8.hip): the append of a packed ragged batch.
 *   rope_kv_append_rows: mm355_rope_kv_append for R rows (on grid.x: R is not bound by 65535): row r of the fused qkv activation is rotated
 *         at positions[r] (the same arithmetic and rounding order), q left in place, rotated k and v written to row positions[r] of block
 *         blocks[r] of the caches [n_blocks][rows_per_block][Hkv*d].  blocks == NULL: block r for row r (needs n_blocks >= R), the bits of
 *         mm355_rope_kv_append; with a table each row's result equals a one-row call of that kernel on its block.  blocks[r] is clamped into
 *         [0, n_blocks) and positions[r] into [0, rows_per_block) (host bounds); no cache row other than the R named ones is written.
 *   rope_kv_append_rows_f8: the twin over an e4m3 cache; quantises exactly as mm355_rope_kv_append_f8 does.
 *   Before any launch: the refusals of mm355_rope_kv_append(_f8); n_blocks < 1 or rows_per_block < 1: MM355_EINVAL.
 * ------------------------------------------------------------------------------------------------ */
int mm355_rope_kv_append_rows(mm355_bf16* qkv, int64_t ld, int64_t R, int64_t Hq, int64_t Hkv, int64_t d, const mm355_bf16* cos_t,
                              const mm355_bf16* sin_t, const int32_t* positions, const int32_t* blocks, int64_t n_blocks,
                              int64_t rows_per_block, mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv,
                              void* stream);
int mm355_rope_kv_append_rows_f8(mm355_bf16* qkv, int64_t ld, int64_t R, int64_t Hq, int64_t Hkv, int64_t d, const mm355_bf16* cos_t,
                                 const mm355_bf16* sin_t, const int32_t* positions, const int32_t* blocks, int64_t n_blocks,
                                 int64_t rows_per_block, uint8_t* k_cache, uint8_t* v_cache, int64_t ld_kv_bytes,
                                 int64_t batch_stride_kv_bytes, float* k_scale, float* v_scale, int64_t ld_scale, int64_t batch_stride_scale,
                                 int fmt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The decode step's attention for B sequences whose first shared_len cached rows are the SAME rows, stored once (csrc/attn_extend_shared.hip):
 * n sampled continuations of one prompt.
 *   attn_decode_shared: q [B][Hq*d] (ld_q), ALREADY rotated; k_shared / v_shared [shared_len][Hkv*d] (row stride ld_shared), one copy;
 *         k_cache / v_cache [B][rows][Hkv*d] as mm355_attn_decode takes them; kv_lens[B] int32 on the device; o [B][Hq*d] (ld_o).  Query row b
 *         attends the keys j in [0, kv_lens[b]): key j < shared_len is row j of k_shared / v_shared, key j >= shared_len is row j of sequence
 *         b's own block (the own rows keep their absolute index, so the append kernels' position is still RoPE position and cache row).  o =
 *         softmax(scale * q K^T) V with the softmax in fp32 and the scale applied on the fp32 side.  kv_lens[b] >= shared_len is the caller's
 *         promise; kv_lens[b] == shared_len (no own rows) and shared_len == 0 are right.  Never read, whatever kv_lens[] says: rows [0,
 *         shared_len) of any sequence's own block, shared rows >= shared_len, own rows >= min(kv_lens[b], max_kv_len).  shared_len and
 *         max_kv_len (shared_len <= max_kv_len <= rows) are host launch parameters.  Shared rows: mm355_attn_extend's kernel with packed row
 *         b * G + g (G = Hq / Hkv), so a shared K / V tile is read once per KV head and 64 / G sequences, the key tiles dealt to several
 *         workgroups; own rows: one more workgroup per (sequence, KV head) in the same launch; a second launch merges the partials.  The
 *         split is a function of (B, Hq, Hkv, shared_len) alone: the same arguments give the same bits.  The workspace
 *         (mm355_attn_decode_shared_ws_floats floats, 16-byte aligned, never 0 for valid arguments) is always needed.
 *   attn_decode_shared_f8: the same over e4m3 bytes and scales, for the shared rows ([shared_len][Hkv] scales, row stride ld_shared_scale) and
 *         the own rows (as mm355_attn_decode_f8 takes them), widened to bf16 on the way into LDS: equal to mm355_attn_decode_shared on the
 *         dequantised cache bit for bit.
 *   Before any launch: fmt other than MM355_KV8_E4M3, a NULL pointer or scale, shared_len < 0 or > max_kv_len, Hq % Hkv != 0, q / o not
 *   16-byte aligned or ld_q / ld_o % 8 != 0, cache pointers or strides not 16-byte (e4m3: 8-byte) aligned, a row stride shorter than a row, a
 *   workspace that is missing or too small: MM355_EINVAL; d % 8 != 0, d > 128 or a GQA group other than 1, 2, 4, 8: MM355_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_attn_decode_shared_ws_floats(int64_t B, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len, int64_t max_kv_len);
int mm355_attn_decode_shared(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared, int64_t ld_shared,
                             const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv,
                             const int32_t* kv_lens, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
                             int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);
int mm355_attn_decode_shared_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared, int64_t ld_shared_bytes,
                                const float* k_shared_scale, const float* v_shared_scale, int64_t ld_shared_scale, const uint8_t* k_cache,
                                const uint8_t* v_cache, int64_t ld_kv_bytes, int64_t batch_stride_kv_bytes, const float* k_scale,
                                const float* v_scale, int64_t ld_scale, int64_t batch_stride_scale, int fmt, const int32_t* kv_lens,
                                int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv,
                                int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same attention with INDEXED own rows: the beams of one prompt (HF GenerationMixin._beam_search, generation/utils.py; the reference
 * reaches it through generate(use_customize_greedy=False, num_beams=K), metamorph_llama.py:711-717, where every step reorders the whole
 * cache).  After a beam step query b continues the hypothesis of some parent beam, so its own rows are scattered over the B blocks; no row
 * moves, a table says where each one lives.
 *   attn_decode_shared_idx / _idx_f8: the arguments of mm355_attn_decode_shared / _f8 plus own_block, a device table of uint8 [B][ld_own_block]
 *         (one byte names a block: B <= 255): for query b, key j >= shared_len is row j of the own block of sequence
 *         own_block[b][j - shared_len]; keys below shared_len are the shared rows.  A NULL table is the identity: mm355_attn_decode_shared's
 *         kernel, bit for bit, and so is the table own_block[b][*] = b.  An entry is the caller's promise; the kernel clamps it into [0, B)
 *         and its column into [0, ld_own_block), so a wrong entry (or a wrong kv_lens[b]) still reads inside the cache and the table.  Never
 *         read: table entries at or beyond min(kv_lens[b], max_kv_len) - shared_len, and everything mm355_attn_decode_shared never reads --
 *         in particular the own rows of blocks the table does not point to.  The e4m3 form follows the table for bytes and scales alike and
 *         equals the bf16 form on the dequantised cache bit for bit.  The shared part, the key split, the merge launch, the workspace
 *         (mm355_attn_decode_shared_ws_floats) and all refusals are mm355_attn_decode_shared's; in addition a table with B > 255 or
 *         ld_own_block < 1 is MM355_EINVAL.  The own workgroup loads the table entries of the tile after next together with the rows of
 *         the next tile, so the dependent load is off the critical path.
 * ------------------------------------------------------------------------------------------------ */
int mm355_attn_decode_shared_idx(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared,
                                 int64_t ld_shared, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                 int64_t batch_stride_kv, const int32_t* kv_lens, const uint8_t* own_block, int64_t ld_own_block,
                                 int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv,
                                 int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);
int mm355_attn_decode_shared_idx_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared,
                                    int64_t ld_shared_bytes, const float* k_shared_scale, const float* v_shared_scale,
                                    int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                    int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                    int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, const uint8_t* own_block,
                                    int64_t ld_own_block, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
                                    int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats,
                                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Extending by n rows per sequence a cache of B sequences whose first shared_len rows are the SAME rows, stored once
 * (csrc/attn_extend_shared.hip): B different questions over one context -- the pass between the prefix and the decode loop.  The union of
 * mm355_attn_extend and mm355_attn_decode_shared.
 *   attn_extend_shared: q [B*n][Hq*d] (ld_q), ALREADY rotated, row (b, i) at b * n + i; k_shared / v_shared [shared_len][Hkv*d] (row stride
 *         ld_shared), one copy; k_cache / v_cache [B][rows][Hkv*d] as mm355_attn_decode takes them; past[B] int32 on the device; o
 *         [B*n][Hq*d] (ld_o).  The own block of sequence b already holds the new rows at past[b] .. past[b] + n - 1 (the append comes first);
 *         past[b] >= shared_len is the caller's promise.  Row (b, i) attends the keys j in [0, shared_len) from the shared copy and then the
 *         keys j in [shared_len, past[b] + i] from row j of block b (the own rows keep their absolute index).  o = softmax(scale * q K^T) V
 *         with the softmax in fp32 and the scale applied on the fp32 side.  Right for n == 1 (mm355_attn_decode_shared's case with kv_lens =
 *         past + 1), shared_len == 0 (mm355_attn_extend's case) and past[b] == shared_len (no earlier own rows).  Never read, whatever past[]
 *         says: rows [0, shared_len) of any own block, shared rows >= shared_len, own rows >= min(past[b] + n, max_kv_len).  shared_len, n and
 *         max_kv_len (shared_len <= max_kv_len <= rows) are host launch parameters.  Shared rows: mm355_attn_decode_shared's shared part with
 *         packed row (b * n + i) * G + g (G = Hq / Hkv), so a shared K / V tile is read once per KV head and 64 / G query rows of any
 *         sequence, the key tiles dealt to several workgroups; own rows: workgroups per (sequence, KV head, 64 packed rows of that
 *         sequence) in the same launch, with mm355_attn_extend's per-row key limit; a second launch merges the partials.  The split is a
 *         function of (B, n, Hq, Hkv, shared_len) alone: the same arguments give the same bits.  The workspace
 *         (mm355_attn_extend_shared_ws_floats floats, 16-byte aligned, never 0 for valid arguments) is always needed.
 *   attn_extend_shared_f8: the same over e4m3 bytes and scales for both parts (as mm355_attn_decode_shared_f8 takes them), widened to bf16 on
 *         the way into LDS: equal to mm355_attn_extend_shared on the dequantised cache bit for bit.
 *   Before any launch: what mm355_attn_decode_shared refuses, with the same codes, and n <= 0 or n > max_kv_len: MM355_EINVAL.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_attn_extend_shared_ws_floats(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len, int64_t max_kv_len);
int mm355_attn_extend_shared(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared, int64_t ld_shared,
                             const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv,
                             const int32_t* past, int64_t n, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
                             int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);
int mm355_attn_extend_shared_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared, int64_t ld_shared_bytes,
                                const float* k_shared_scale, const float* v_shared_scale, int64_t ld_shared_scale, const uint8_t* k_cache,
                                const uint8_t* v_cache, int64_t ld_kv_bytes, int64_t batch_stride_kv_bytes, const float* k_scale,
                                const float* v_scale, int64_t ld_scale, int64_t batch_stride_scale, int fmt, const int32_t* past, int64_t n,
                                int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv,
                                int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise: SwiGLU (HF LlamaMLP; K12), GELU (projector / vision_head), scaling helpers.
 * gu = [M][2I] with gate in columns [0,I) and up in [I,2I).
 * ------------------------------------------------------------------------------------------------ */
int mm355_swiglu_fwd(const mm355_bf16* gu, mm355_bf16* act, int64_t M, int64_t I, void* stream);
int mm355_swiglu_bwd(const mm355_bf16* gu, const mm355_bf16* dact, mm355_bf16* dgu, mm355_bf16* act,
                     int64_t M, int64_t I, void* stream);
/* same, additionally emitting the contraction-major copies the weight-gradient GEMMs consume: actT[I][M] and dguT[2I][M]
 * (what mm355_transpose_bf16 would make of act and dgu).  M % 64 == 0 and I % 64 == 0, else MM355_EUNSUPPORTED. */
int mm355_swiglu_bwd_t(const mm355_bf16* gu, const mm355_bf16* dact, mm355_bf16* dgu, mm355_bf16* actT,
                       mm355_bf16* dguT, int64_t M, int64_t I, void* stream);
#define MM355_GELU_ERF  0
#define MM355_GELU_TANH 1
int mm355_gelu_fwd(const mm355_bf16* x, mm355_bf16* y, int64_t n, int kind, void* stream);
int mm355_gelu_bwd(const mm355_bf16* x, const mm355_bf16* dy, mm355_bf16* dx, int64_t n, int kind, void* stream);
/* x[i] *= *s_dev (optionally times s_host) */
int mm355_scale_bf16(mm355_bf16* x, int64_t n, const float* s_dev, float s_host, void* stream);
/* y[i] (+)= s * x[i]; y bf16, x bf16/f32 */
int mm355_axpy_bf16(mm355_bf16* y, const mm355_bf16* x, int64_t n, const float* s_dev, float s_host,
                    int accumulate, void* stream);
int mm355_axpy_f32_to_bf16(mm355_bf16* y, const float* x, int64_t n, float s_host, int accumulate, void* stream);
/* the same with a DEVICE scalar on top (s_dev nullable): y (+)= s_dev[0] * s_host * x -- fp32-accumulated lm_head weight gradient
 * scaled by the upstream loss gradient without a host sync (functional.LinearCrossEntropyFn) */
int mm355_axpy_f32_to_bf16_dev(mm355_bf16* y, const float* x, int64_t n, const float* s_dev, float s_host, int accumulate,
                               void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cross entropy over a chunk of rows of bf16 logits (metamorph_llama.py:398-413; K13).
 * logits [R][ld] bf16 (columns [V,ld) are padding).  targets[r] in [0,V) or < 0 = ignored row.
 * loss_sum += sum_r (lse_r - logit_r[target]);  then, IN PLACE, logits <- grad_scale*(softmax - onehot)
 * (zero on ignored rows and padding columns).  fp32 math on the bf16-rounded logits like the reference's
 * `.float()`; rows are compacted by the host so ignored rows normally never reach this kernel.
 * row_ws (nullable, R floats): the per-row NLL values are written there and added to loss_sum in a FIXED order by one workgroup
 * (bit-reproducible loss); NULL = one fp32 atomicAdd per row (order, hence the last bits, vary from run to run).  The same parameter
 * exists on the three image-AR loss entry points below.  loss_sum may be NULL when row_ws is given (per-row values only).
 * ------------------------------------------------------------------------------------------------ */
int mm355_ce_rows(mm355_bf16* logits, int64_t ld, const int32_t* targets, int64_t R, int64_t V,
                  float grad_scale, float* loss_sum, float* row_ws, void* stream);
/* out[0] = (accumulate ? out[0] : 0) + scale * sum(values[0..n)) in a fixed order (one workgroup; the reduction behind row_ws) */
int mm355_sum_rows_f32(const float* values, int64_t n, float scale, float* out, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * lm_head + shifted cross entropy, forward and both gradients, as ONE call (SURVEY 8(b) `linear_ce`; reference metamorph_llama.py:393-413:
 * `logits = lm_head(hidden).float()`, shift, `CrossEntropyLoss()` = mean NLL over the positions whose next label is live).
 *   hidden [*, ldh] bf16 rows of the final-norm output; rows[i] (int32, device; NULL = rows 0..n-1) = the row that predicts targets[i]
 *   (int32, device, in [0, V)) -- the host plan lists only positions with a live next label, so no flop is spent on ignored ones;
 *   W [V, ldw] = lm_head.weight.
 *   loss[0]        = (1/n) sum_i NLL_i, the per-row values summed in a fixed order (bit-reproducible);
 *   d_hidden [n,h] = d loss / d hidden[rows[i]] (compact, bf16; NULL = not wanted);
 *   dW [V,h]       = d loss / d W, OVERWRITTEN (bf16, or fp32 when dw_f32 != 0; NULL = not wanted).
 * The rows go through the logits GEMM in chunks of 8192: bf16 logits (the reference's bf16 nn.Linear output) -> mm355_ce_rows (fp32 math,
 * gradient in place) -> the two gradient GEMMs; the [n, V] fp32 logits tensor never exists.  Workspace: mm355_linear_ce_ws_bytes(n, V, h,
 * gather = rows != NULL, need_dh = d_hidden != NULL, need_dw = dW != NULL) bytes, 16-byte aligned.
 * ------------------------------------------------------------------------------------------------ */
int64_t mm355_linear_ce_ws_bytes(int64_t n, int64_t V, int64_t h, int gather, int need_dh, int need_dw);
int mm355_linear_ce(const mm355_bf16* hidden, int64_t ldh, const int32_t* rows, const int32_t* targets, int64_t n,
                    const mm355_bf16* W, int64_t ldw, int64_t V, int64_t h, float* loss, mm355_bf16* d_hidden, void* dW,
                    int dw_f32, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Splice (metamorph_arch.py:259-399; K6) driven by the host gather plan (bit-exact int bookkeeping):
 *   src[r] >= 0        -> row src[r] of embed_tokens.weight
 *   src[r] == -1       -> zero row (padding)
 *   src[r] <= -2       -> row (-2 - src[r]) of the projected image features
 * ------------------------------------------------------------------------------------------------ */
int mm355_splice_gather(const mm355_bf16* embed, const mm355_bf16* proj, const int32_t* src,
                        mm355_bf16* out, int64_t rows, int64_t h, void* stream);
/* backward into the projector output: dproj[n] = dout[row_of_feature[n]] or 0 when row_of_feature[n] < 0 */
int mm355_rows_gather(const mm355_bf16* in, int64_t ld_in, const int32_t* idx, mm355_bf16* out, int64_t ld_out,
                      int64_t R, int64_t h, void* stream);
/* dst[idx[r]] += src[r]   (idx unique) */
int mm355_rows_scatter_add(const mm355_bf16* src, int64_t ld_src, const int32_t* idx, mm355_bf16* dst,
                           int64_t ld_dst, int64_t R, int64_t h, void* stream);
/* embedding gradient: for segment s (token id tok[s]) sum rows pos[seg_start[s] .. seg_start[s+1]) of dout
 * in fp32 and (accumulate ? add to : store as) dembed[tok[s]].  Deterministic, no atomics. */
int mm355_embed_grad(const mm355_bf16* dout, const int32_t* tok, const int32_t* seg_start, const int32_t* pos,
                     int64_t n_seg, mm355_bf16* dembed, int64_t h, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Vision front/back ends.
 * im2col: images [N][3][H][W] (f32 or bf16) -> patches [N*gh*gw][Kp] bf16, k = c*p*p + dy*p + dx,
 *         columns [3*p*p, Kp) zero  (SigLIP patch embedding Conv2d 14x14/14, "valid"; K1).
 * bilinear_l2norm: [N][side_in^2][C] -> [N][side_out^2][C]; fp32 bilinear (align_corners=False), round to
 *         bf16, then F.normalize(p=2, eps 1e-12) in bf16 when normalize != 0 (siglip_encoder.py:151-163,206-208).
 * ------------------------------------------------------------------------------------------------ */
int mm355_im2col_patch(const void* images, int images_are_f32, int64_t N, int64_t H, int64_t W, int64_t p,
                       mm355_bf16* out, int64_t Kp, void* stream);
int mm355_bilinear_l2norm(const mm355_bf16* in, mm355_bf16* out, int64_t N, int64_t side_in, int64_t side_out,
                          int64_t C, int normalize, void* stream);
/* backward of the above for a trainable tower (freeze_vision=False, siglip_encoder.py:139): d_in_f32[N][side_in^2][C] +=
 * scatter of d/d(interpolated row) with the bilinear weights (caller zeroes d_in_f32; fp32 atomics). */
int mm355_bilinear_l2norm_bwd(const mm355_bf16* in, const mm355_bf16* d_out, float* d_in_f32, int64_t N, int64_t side_in,
                              int64_t side_out, int64_t C, int normalize, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Cosine regression loss (metamorph_llama.py:433-435,449-455; K16).  pred_raw = vision_head output.
 *   p = normalize ? F.normalize(pred_raw) (bf16 rounded) : pred_raw
 *   loss_sum += sum_r cos(target_r, p_r)  (caller turns it into -mean);  dpred = d(-mean cos)/d pred_raw * 1
 * ------------------------------------------------------------------------------------------------ */
int mm355_cosine_loss(const mm355_bf16* pred_raw, const mm355_bf16* target, int64_t R, int64_t C, int normalize,
                      float* cos_sum, mm355_bf16* dpred, float* row_ws, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The other two image-AR head variants (metamorph_llama.py:437-447 soft-CE, :459 + :211-219 mean-abs) and the
 * temperature softmax they pair with on the tower side (siglip_encoder.py:210-211) and in image-mode decoding
 * (metamorph_llama.py:372-373).  One wave per row, C % 8 == 0.
 *   mean_abs:  abs_sum[0] += sum |target - pred| (bf16 difference like the reference stack); caller divides by R*C.
 *              dpred (nullable) = d mean|t - p| / d pred.     (constructor default: normalize_vision=False, apply_softmax=False)
 *   soft_ce:   u = normalize ? F.normalize(pred_raw) : pred_raw;  q = softmax(u / temperature) (bf16);
 *              loss_sum[0] += -sum_r sum_j target[r][j] log(q[r][j] + 1e-10); caller divides by R.
 *              dpred (nullable) = d (loss_sum / R) / d pred_raw.
 *   softmax_rows:     y = softmax(x / temperature) per row (fp32 inside, bf16 out).
 *   softmax_rows_bwd: dx = y * (dy - sum_j dy_j y_j) / temperature.
 * ------------------------------------------------------------------------------------------------ */
int mm355_mean_abs_loss(const mm355_bf16* pred, const mm355_bf16* target, int64_t R, int64_t C, float* abs_sum,
                        mm355_bf16* dpred, float* row_ws, void* stream);
int mm355_soft_ce_loss(const mm355_bf16* pred_raw, const mm355_bf16* target, int64_t R, int64_t C, int normalize,
                       float temperature, float* loss_sum, mm355_bf16* dpred, float* row_ws, void* stream);
int mm355_softmax_rows(const mm355_bf16* x, mm355_bf16* y, int64_t R, int64_t C, float temperature, void* stream);
int mm355_softmax_rows_bwd(const mm355_bf16* y, const mm355_bf16* dy, mm355_bf16* dx, int64_t R, int64_t C,
                           float temperature, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The greedy loop's per-token tail on the device (metamorph_llama.py:502-597): with these the host reads nothing per token.
 * argmax_rows_f32: out[r] (int32) = argmax of row r of the contiguous fp32 logits x [R, C], torch.argmax's rule: among equal maxima the
 *         lowest index, a NaN beats every number, the lowest NaN index.  Two stages in fixed order (one partial per row and 4096-column
 *         chunk, then one reduction per row), no atomics; workspace: mm355_argmax_rows_ws_bytes(R, C) bytes, 4-byte aligned.
 * rows_select_bf16: out[r] = mask[r] ? a[r] : b[r] (int32 mask on the device; h % 8 == 0, 16-byte aligned rows): the lm_head input per
 *         sequence, the projector row in image mode (:363-377), the normed hidden row otherwise.
 * greedy_advance: one workgroup per sequence runs the loop's branch (:569-589) on device-resident state (int32 [B] each: in_image, n_img,
 *         total_out, done, n_tokens, n_z) with tok[b] = this step's argmax:
 *           done:                            nothing is written (state, logs and the x_in row stay)
 *           !in_image && tok == start_id:    in_image = 1; log tok; next row = embed[tok]
 *           in_image && n_img < N:           n_img++; log pred_z[b]; next row = fed[b] (the row the lm_head saw); n_img == N: in_image = 0
 *           tok == end_id:                   in_image = 0; n_img = 0; log tok; next row = embed[tok]
 *           else:                            log tok; next row = embed[tok]
 *           total_out++; tok among the eos ids or total_out > max_new_tokens: done = 1
 *         Writes row b of x_in [B, h], tok_log [B, token_cap] int32, z_log [B, z_cap, Dz] bf16 and decrements live[0] (sequences not yet
 *         done; the caller initialises it) when a sequence finishes.  A log row at or beyond its cap is never written: the sequence is set
 *         done instead and nothing else changes.  C (the logits width tok comes from) > embed_rows is MM355_EINVAL, so every id used as a
 *         gather index lies in [0, embed_rows).  eos_ids: HOST memory, n_eos <= MM355_GREEDY_MAX_EOS.
 *         The host-side model of the transition is metamorph_amd.functional.greedy_advance_host.
 * ------------------------------------------------------------------------------------------------ */
#define MM355_GREEDY_MAX_EOS 8
int64_t mm355_argmax_rows_ws_bytes(int64_t R, int64_t C);
int mm355_argmax_rows_f32(const float* x, int64_t R, int64_t C, int32_t* out, void* workspace, int64_t workspace_bytes,
                          void* stream);
int mm355_rows_select_bf16(const mm355_bf16* a, int64_t lda, const mm355_bf16* b, int64_t ldb, const int32_t* mask,
                           mm355_bf16* out, int64_t ldo, int64_t R, int64_t h, void* stream);
int mm355_greedy_advance(const int32_t* tok, int64_t B, int64_t C, int32_t* in_image, int32_t* n_img, int32_t* total_out,
                         int32_t* done, int32_t* n_tokens, int32_t* n_z, int32_t* live, const mm355_bf16* embed,
                         int64_t ld_embed, int64_t embed_rows, const mm355_bf16* fed, int64_t ld_fed, const mm355_bf16* pred_z,
                         int64_t ld_z, mm355_bf16* x_in, int64_t ld_x, int64_t h, int64_t Dz, int32_t* tok_log,
                         int64_t token_cap, mm355_bf16* z_log, int64_t z_cap, int start_id, int end_id, int num_image_tokens,
                         int max_new_tokens, const int32_t* eos_ids, int n_eos, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sampled decoding in the same loop: the two kernels that stand where argmax_rows_f32 stands (functional.GreedyLoopGraph(sampler=...)).
 * philox_uniform_rows: u[r] = (word 0 of Philox4x32-10 with key (seed low 32, seed high 32) and counter (counters[r], stream_ids[r], 0, 0)
 *         >> 8) * 2^-24, in [0, 1); stream_ids, counters (int32, read as uint32) and u are device arrays of R entries.  Stateless: a draw
 *         is a function of (seed, stream id, counter) alone -- in the loop the counter is the sequence's total_out, so warm-up launches,
 *         captures, polling and the batch a sequence rides in cannot move it.  The host model: functional.philox_uniform_host.
 * sample_rows_f32: out[r] (int32) = one draw from row r of the contiguous fp32 logits x [R, C] (bounds on R and C as for argmax_rows_f32)
 *         under HF's temperature -> top-k -> top-p -> multinomial, written without a sort.  With m the row maximum:
 *           m NaN, +inf or -inf:  out[r] = argmax_rows_f32's index, stats = (m, 0)
 *           w_i = exp((x_i - m) * inv_temperature) in fp32 (v_exp_f32: a few 1e-6 relative); -inf weighs 0
 *           top-k:  i is kept iff #{j: x_j > x_i} < top_k (0 or >= C: off; ties at the k-th value are all kept)
 *           top-p:  of those, i is kept iff sum_{x_j > x_i} w_j < top_p * sum_{kept by top-k} w_j (>= 1: off; the maximum is always kept)
 *           so the kept set is {x_i >= tau}, tau a value of the row (no filter: its minimum); Z = sum of w over it
 *           out[r] = the smallest kept i with w_0 + .. + w_i (kept terms, index order) > u[r] * Z; if rounding leaves none, the last kept i
 *         stats (nullable, fp32 [R, 2]) receives (tau, Z).  One workgroup per row, so a row's result is a bit-reproducible function of the
 *         row, u[r] and the scalars, whatever R and the other rows are.  tau comes from two 5-round selects (256 linear bins over the
 *         row's range, then the four bytes of an order-preserving key) on integer LDS histograms: counts for top-k, weights in fixed point
 *         (w * 2^40, exact integer sums) for top-p, whose boundary can therefore sit one token off the fp32 one where the mass above a
 *         token is within ~1e-6 * Z of top_p * Z.  Z and the pick's prefixes are fp32 trees (per-lane partials over C / 16384 terms,
 *         wave butterflies, 16 chunk sums per wave and the 16 wave sums in index order); no floating-point atomics anywhere.  The workspace is unused by this one-workgroup
 *         form (sample_rows_ws_bytes returns 0, workspace may be null); inv_temperature not finite or <= 0, top_k < 0, top_p outside
 *         (0, 1]: MM355_EINVAL.  The host model: functional.sample_row_host.
 * ------------------------------------------------------------------------------------------------ */
int mm355_philox_uniform_rows(uint64_t seed, const int32_t* stream_ids, const int32_t* counters, float* u, int64_t R, void* stream);
int64_t mm355_sample_rows_ws_bytes(int64_t R, int64_t C);
int mm355_sample_rows_f32(const float* x, int64_t R, int64_t C, float inv_temperature, int top_k, float top_p, const float* u,
                          int32_t* out, float* stats, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Logits processors and per-token log-probabilities in the same loop (functional.GreedyLoopGraph(processors=...)).  Both kernels run one
 * workgroup per row of the contiguous fp32 logits x [R, C] (bounds on R and C as for argmax_rows_f32), use no floating-point atomics and
 * read no host value at run time (they can be captured); a row's result is a bit-reproducible function of that row's inputs, whatever R
 * and the other rows are.  `seen` is a device bitmap, uint32 [R, seen_words], seen_words >= ceil(C / 32): bit (i & 31) of word (i >> 5)
 * of row r is id i of sequence r; bits at positions >= C are ignored, whatever they hold.
 * logits_process_rows_f32: edits x in place, per row in HF's order (RepetitionPenaltyLogitsProcessor, MinNewTokensLengthLogitsProcessor,
 *         SuppressTokensLogitsProcessor):
 *           1. every i < C whose bit is set:  x_i = x_i < 0 ? x_i * penalty : x_i / penalty, in fp32 with a correctly rounded division
 *              (NaN stays NaN, -0.0 stays -0.0, +-inf keep their sign); skipped when penalty == 1 or seen is null
 *           2. min_new_tokens > 0 and total_out[r] (int32 [R], the loop's state row) < min_new_tokens:  x[e] = -inf for every eos id e
 *           3. x[s] = -inf for every id s of suppress_ids (int32, DEVICE memory, n_suppress entries, any length)
 *         Ids outside [0, C) in either list are skipped and never cause a write outside the row; an entry that is neither marked nor
 *         listed keeps its bits.  eos_ids: HOST memory, n_eos <= MM355_GREEDY_MAX_EOS, as for greedy_advance.  With nothing to edit no
 *         kernel is launched.  MM355_EINVAL before any launch: x null, R or C out of bounds, penalty not finite or <= 0, penalty != 1
 *         with a null seen, seen_words < ceil(C / 32) (penalty != 1), min_new_tokens > 0 with a null total_out, n_eos above the cap or
 *         n_eos > 0 with a null list, n_suppress < 0 or n_suppress > 0 with a null list.  The host model, which the kernel equals bit for
 *         bit: functional.logits_process_host.
 * token_note_rows_f32: runs after the pick (tok [R], the id argmax_rows_f32 or sample_rows_f32 wrote) and BEFORE greedy_advance, on the
 *         state greedy_advance is about to read (in_image, n_img, done, n_tokens: int32 [R] each).  Row r logs an id iff !done[r] and
 *         !(in_image[r] && n_img[r] < num_image_tokens) and n_tokens[r] < token_cap and 0 <= tok[r] < C -- the rows for which
 *         greedy_advance writes tok_log[r][n_tokens[r]].  For such a row:
 *           seen (nullable):      the bit of tok[r] is set (one thread's read-modify-write of one word)
 *           logp_log (nullable, fp32 [R, token_cap]):  logp_log[r][n_tokens[r]] = x[tok] - m - ln(sum_i exp(x_i - m)), m the row maximum,
 *                                 -inf entries weigh 0; a NaN in the row, m = +inf or m = -inf (a row of -inf only): NaN; x[tok] = -inf
 *                                 under a finite m: -inf
 *         For every other row nothing is written anywhere.  The log-probability is that of the row the kernel finds in x: the PROCESSED
 *         logits (after logits_process_rows_f32, before temperature, top-k and top-p); with no processor active it is the model's own
 *         log-softmax.  exp is v_exp_f32 (a few 1e-6 relative), the sum a fixed-order fp32 tree (thread t of 1024 adds the columns
 *         t, t + 1024, ... in that order, then the wave butterflies and the 16 wave sums in index order): within 1e-4 + 2^-22 |logp| of
 *         the fp64 value.  MM355_EINVAL: a null x, tok or state row, R or C out of bounds, token_cap outside [0, INT_MAX], seen and
 *         logp_log both null, seen with seen_words < ceil(C / 32).  The host model: functional.token_note_host.
 * ------------------------------------------------------------------------------------------------ */
int mm355_logits_process_rows_f32(float* x, int64_t R, int64_t C, float penalty, const uint32_t* seen, int64_t seen_words,
                                  const int32_t* total_out, int min_new_tokens, const int32_t* eos_ids, int n_eos,
                                  const int32_t* suppress_ids, int64_t n_suppress, void* stream);
int mm355_token_note_rows_f32(const float* x, int64_t R, int64_t C, const int32_t* tok, const int32_t* in_image, const int32_t* n_img,
                              const int32_t* done, const int32_t* n_tokens, int num_image_tokens, int64_t token_cap, uint32_t* seen,
                              int64_t seen_words, float* logp_log, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Beam search in the same loop (functional.BeamLoopGraph; csrc/beam.hip): HF's GenerationMixin._beam_search (transformers
 * generation/utils.py, which the reference reaches through generate(use_customize_greedy=False, num_beams=K), metamorph_llama.py:711-717)
 * for ONE prompt, do_sample=False, no logits processors.  K <= MM355_BEAM_MAX beams, V logits, M = max(2, 1 + eos ids) * K candidates.
 * Both entry points read no host value at run time (they can be captured), use no floating-point atomics and are bit-reproducible
 * functions of their inputs; all arithmetic is fp32 with HF's literal -1e9.
 * beam_select_rows_f32: x [K, V] contiguous fp32 logits, running [K] the beams' scores (no NaN).  Writes
 *           stats [K, 2] = (row maximum m, lse = ln sum_i exp(x_i - m)), computed as token_note_rows_f32 computes them (v_exp_f32, the same
 *                 fixed-order tree; within 1e-4 + 2^-22 |value| of fp64); a NaN in the row, m = +inf or m = -inf: lse = NaN
 *           cand_val [M], cand_idx [M]: the M best of acc[b * V + i] = ((x[b,i] - m_b) - lse_b) + running[b], the operations in exactly
 *                 that fp32 order, sorted by value descending, a NaN after every number (a row whose lse is NaN has NaN scores
 *                 throughout), among equals the lower flat index first
 *         One workgroup per row finds the row's min(M, V) best (the M best of all lie among them): the min(M, V)-th largest of the 1024
 *         per-thread maxima bounds them from below, what reaches the bound goes through an exact radix select on (order-preserving value
 *         key, index) pairs with integer LDS histograms; a second launch of one workgroup ranks the K * min(M, V) partial candidates.
 *         workspace: mm355_beam_select_rows_ws_bytes(K, V, M) bytes, 4-byte aligned.  MM355_EINVAL before any launch: a null pointer, K
 *         outside [1, MM355_BEAM_MAX], M outside [K, 9 K] or > K V, V < 1 or beyond argmax_rows_f32's bound, a workspace too small.
 *         The host model: functional.beam_select_host.
 * beam_advance: one launch runs HF's step on the M sorted candidates (candidate c: parent = idx / V, id = idx % V; an idx outside [0, K V)
 *         is clamped into it) and device-resident state: running [K] fp32 (start: 0, -1e9, ...), fin_score [K] fp32 (start: -1e9),
 *         fin_flag [K] int32 (0), fin_end [K, 3] int32, scal [2] int32 = (heuristic unsatisfied: 1, generated length n: 0), live [1] (1).
 *           hit[c] = id among the eos ids, or n + 1 >= max_new_tokens
 *           running beams: the K best of val + hit * -1e9 -> running, tok [K], parent [K], row n of tok_log / parent_log [log_cap, K]
 *           pool: the K best of (old pool, val / len_pow[n] - 1e9 [pool full and early_stopping == 1] - 1e9 [heuristic satisfied]
 *                 - 1e9 [not (hit and c < K)]), three successive additions; flags travel with the scores and fin_end of an entry says
 *                 where its hypothesis ended: (step n, the parent's slot, id) -- the host rebuilds the ids from the back-pointer logs
 *           n += 1; unsatisfied &= any_k(running[0] / len_pow[L - 1] > (fin_flag[k] ? min(fin_score) : -1e9)), L = max_new_tokens if
 *                 early_stopping == 2 ("never") and length_penalty > 0, else n
 *           live[0] = 0 unless unsatisfied and not (all flags and early_stopping == 1) and not all M candidates hit
 *           own_block (nullable, uint8 [K, ld_own_block], the table of mm355_attn_decode_shared_idx): column t < n of slot i becomes that
 *                 of slot parent[i] (a column is read whole before it is written: in place), column n becomes i -- the row slot i
 *                 itself appends in the next decode step, in its own block
 *           x_in (nullable together with embed): row i = embed[tok[i]]
 *         Ties in the three selections go to the lower index (torch.topk leaves them open), a NaN sorts last.  len_pow: DEVICE fp32
 *         [max_new_tokens], len_pow[t - 1] = (float)(t ** length_penalty), made on the host: the device calls no pow.  With live[0] == 0
 *         the launch writes nothing, so a finished search rides along as finished sequences do in greedy_advance; n outside [0,
 *         max_new_tokens) sets live[0] = 0 and writes nothing else.  eos_ids: HOST memory, n_eos <= MM355_GREEDY_MAX_EOS.  MM355_EINVAL:
 *         a null pointer (own_block and the embed / x_in pair excepted), K, M, V as above, max_new_tokens < 1, log_cap or ld_own_block <
 *         max_new_tokens, early_stopping outside {0, 1, 2}, a NaN length_penalty, V > embed_rows, rows that are not 16-byte vectors.
 *         The host model: functional.beam_step_host.
 * ------------------------------------------------------------------------------------------------ */
#define MM355_BEAM_MAX 8
int64_t mm355_beam_select_rows_ws_bytes(int64_t K, int64_t V, int64_t M);
int mm355_beam_select_rows_f32(const float* x, int64_t K, int64_t V, const float* running, int64_t M, float* stats, float* cand_val,
                               int32_t* cand_idx, void* workspace, int64_t workspace_bytes, void* stream);
int mm355_beam_advance(const float* cand_val, const int32_t* cand_idx, int64_t K, int64_t M, int64_t V, float* running, float* fin_score,
                       int32_t* fin_flag, int32_t* fin_end, int32_t* scal, int32_t* live, int32_t* tok, int32_t* parent, int32_t* tok_log,
                       int32_t* parent_log, int64_t log_cap, uint8_t* own_block, int64_t ld_own_block, const mm355_bf16* embed,
                       int64_t ld_embed, int64_t embed_rows, mm355_bf16* x_in, int64_t ld_x, int64_t h, const float* len_pow,
                       int max_new_tokens, float length_penalty, int early_stopping, const int32_t* eos_ids, int n_eos, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prompt-lookup speculative decoding in the greedy device loop (csrc/spec.hip, functional.SpecGreedyLoopGraph; HF's
 * prompt_lookup_num_tokens).  A step carries n = K + 1 rows per sequence through the decoder, row (b, i) at b * n + i: row 0 is the
 * sequence's real next input, rows 1 .. n_draft[b] the embeddings of guessed next ids, the rest dummies.  Row (b, i) is appended at cache
 * row pos[b] + i and sees the rows before it (mm355_rope_kv_append_rows, mm355_attn_extend), so its argmax is the loop's next id whenever
 * the guesses before it were right.  One workgroup per sequence in both kernels; no atomics but the decrement of live[0], which is
 * mm355_greedy_advance's.
 * ngram_draft_rows: the guesses.  hist [B, hist_cap] int32 holds what a sequence's drafts are looked up in -- its lookup ids (any int32:
 *         the -200 image sentinel stays in) followed by the ids it has logged --, hist_len [B] how many.  The rule is
 *         PromptLookupCandidateGenerator.get_candidates with no eos ids, no logits processor and no max_length:
 *           for m = min(N, len - 1) .. 1: the pattern is the last m ids; among the indices idx < len - m where it occurs, the LOWEST whose
 *           continuation hist[idx + m : min(idx + m + K, len)], cropped at the first id outside [0, C), is not empty gives the drafts
 *           (the trailing occurrence has none; a match whose continuation begins outside [0, C) is skipped); the first m with such an
 *           index wins; none: 0 drafts.  A sequence whose in_image is set gets 0 drafts; for one that is done only pos_rows is written (its rows
 *           keep landing at and above its length; the loop's warm-up and capture run with every sequence done and must leave the first
 *           step's drafts alone, and pos_rows is then what it was).
 *         The scan is strided over the workgroup (any len), the minimum over the hits taken in fixed order.  Writes drafts [B, K] (-1
 *         behind the drafts), n_draft [B], and the step's input: x_in row b * n + 1 + j = embed[drafts[b][j]] for j < n_draft[b] and a
 *         row of zeros for the other j < K (row b * n is NOT written: it is the advance kernel's), pos_rows[b * n + i] = pos[b] + i,
 *         mask_rows[b * n + i] = in_image[b] for i == 0, else 0 (the head's row select).  Writes none of the loop's state.
 *         The host model: functional.prompt_lookup_host.
 * spec_verify_advance: tok [B * n] = the argmax of every row.  For i = 0, 1, ... ONE iteration of mm355_greedy_advance's transition
 *         (functional.greedy_advance_host) with tok[b * n + i], fed / pred_z taken from row b * n + i, the logs and caps as there.  The
 *         iteration is counted, and the walk ends at the first of: it logged nothing (a full log: the sequence is set done); the
 *         sequence is now done; it was an image row (the next input is a fed row, not an id's embedding); the sequence is now in image
 *         mode (the next row's head mask differs); i == n_draft[b]; tok != drafts[b][i].  With a iterations counted: the logged ids are
 *         appended to hist (hist_len advances; a full hist is left as it is), x_in row b * n becomes what mm355_greedy_advance would
 *         write after the last logging iteration, and, count_step != 0: pos[b] += a, len[b] += a (the cache's write position and
 *         visible length: rows pos .. pos + a - 1 of this step were right inputs), acc_log[b][n_steps[b]++] = a (acc_log [B, acc_cap]; a
 *         full log row is left).  count_step == 0: the loop's first iteration, run on the prompt's last hidden row without a decoder
 *         step -- no cache row was appended, pos / len / acc_log / n_steps are not touched (and may be NULL).  A sequence that is done
 *         on entry writes NOTHING: a finished sequence's cache length stands still.  live[0] is decremented when a sequence finishes.
 *         eos_ids: HOST memory.  The host model: functional.spec_advance_host, a loop over greedy_advance_host.
 * MM355_EINVAL before any launch: a null pointer, K outside [1, MM355_SPEC_MAX_DRAFT], N outside [1, MM355_SPEC_MAX_NGRAM], B < 1, C < 1
 * or > embed_rows, hist_cap < 1, h % 8 or Dz % 8 != 0, rows that are not 16-byte vectors, more than MM355_GREEDY_MAX_EOS eos ids.
 * ------------------------------------------------------------------------------------------------ */
#define MM355_SPEC_MAX_DRAFT 15
#define MM355_SPEC_MAX_NGRAM 8
int mm355_ngram_draft_rows(const int32_t* hist, int64_t hist_cap, const int32_t* hist_len, const int32_t* done, const int32_t* in_image,
                           const int32_t* pos, int64_t B, int K, int N, int64_t C, const mm355_bf16* embed, int64_t ld_embed,
                           int64_t embed_rows, int32_t* drafts, int32_t* n_draft, mm355_bf16* x_in, int64_t ld_x, int64_t h,
                           int32_t* pos_rows, int32_t* mask_rows, void* stream);
int mm355_spec_verify_advance(const int32_t* tok, const int32_t* drafts, const int32_t* n_draft, int64_t B, int K, int64_t C,
                              int32_t* in_image, int32_t* n_img, int32_t* total_out, int32_t* done, int32_t* n_tokens, int32_t* n_z,
                              int32_t* live, const mm355_bf16* embed, int64_t ld_embed, int64_t embed_rows, const mm355_bf16* fed,
                              int64_t ld_fed, const mm355_bf16* pred_z, int64_t ld_z, mm355_bf16* x_in, int64_t ld_x, int64_t h,
                              int64_t Dz, int32_t* tok_log, int64_t token_cap, mm355_bf16* z_log, int64_t z_cap, int32_t* hist,
                              int64_t hist_cap, int32_t* hist_len, int32_t* pos, int32_t* len, int32_t* acc_log, int64_t acc_cap,
                              int32_t* n_steps, int count_step, int start_id, int end_id, int num_image_tokens, int max_new_tokens,
                              const int32_t* eos_ids, int n_eos, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ZeRO-2 shard update (replaces DeepSpeed zero2.json + HF adamw_torch, train.py:82): AdamW on the
 * rank's fp32 master shard, writes the updated bf16 parameters.  grad_scale_dev (nullable) is a device
 * scalar multiplied into the gradient (1/world, clip coefficient).
 * ------------------------------------------------------------------------------------------------ */
int mm355_adamw_shard(float* p32, float* m, float* v, const mm355_bf16* g, mm355_bf16* p_out, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay,
                      float bias_corr1, float bias_corr2, const float* grad_scale_dev, void* stream);
/* out[0] += sum x^2 (grad-norm partial).  Deterministic (no atomics): per-workgroup sums go to `partials` (caller-allocated,
 * MM355_SUMSQ_PARTIALS floats, contents scratch) and are added in index order by a second one-workgroup launch. */
#define MM355_SUMSQ_PARTIALS 2048
int mm355_sumsq_bf16(const mm355_bf16* x, int64_t n, float* out, float* partials, void* stream);
/* clip coefficient: coef[0] = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)) * pre_scale */
int mm355_clip_coef(const float* sumsq, float max_norm, float pre_scale, float* coef, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MM355_H */

// The second launch of a split-K projection, shared by the bf16 split-K GEMM (gemm_bf16.hip, where the kernels live) and its e4m3 and MXFP4
// twins (gemm_w8.hip, gemm_w4.hip): fp32 partials [slices][M][N] -> the bf16 result, alone or with what follows the projection on the decode / prompt path.
// Library-internal: none of these is part of the C ABI.
#pragma once
#include "mm355_common.h"

#define MM_INTERNAL __attribute__((visibility("hidden")))

// K slices of an M x N x K prompt-pass problem (1: not split)
MM_INTERNAL int mm_splitk_slices(int64_t M, int64_t N, int64_t K);
// floats of workspace a projection needs (the *_ws_floats queries of every format): the partials of a split problem ...
static inline int64_t mm_splitk_ws_floats(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, N, K);
    return S > 1 ? (int64_t)S * M * N : 0;
}
// ... and for the SwiGLU forms, not split: the bf16 [M][2 I] gate | up rows of the plain sequence
static inline int64_t mm_splitk_swiglu_ws_floats(int64_t M, int64_t I, int64_t K) {
    if (M <= 0 || I <= 0 || K <= 0) return 0;
    const int S = mm_splitk_slices(M, 2 * I, K);
    return S > 1 ? (int64_t)S * M * 2 * I : M * I;
}
// C = bf16(sum_s part[s] (+ residual)), slices added in order
MM_INTERNAL int mm_splitk_reduce(const float* part, int slices, int64_t M, int64_t N, const mm355_bf16* residual, int64_t ldr, mm355_bf16* C,
                                 int64_t ldc, hipStream_t stream);
// ... and Y = RMSNorm(C; norm_w, eps); C and Y rows N apart.  N / 8 <= 2048 (the caller checks)
MM_INTERNAL int mm_splitk_reduce_norm(const float* part, int slices, int64_t M, int64_t N, const mm355_bf16* residual, int64_t ldr, mm355_bf16* C,
                                      const mm355_bf16* norm_w, float eps, mm355_bf16* Y, hipStream_t stream);
// act = SiLU(g) * u of the bf16-rounded sums, N = 2 I
MM_INTERNAL int mm_splitk_reduce_swiglu(const float* part, int slices, int64_t M, int64_t I, mm355_bf16* act, int64_t ld_act, hipStream_t stream);
// q rotated -> qkv, rotated k and v -> the cache rows positions[m]
MM_INTERNAL int mm_splitk_reduce_rope_append(const float* part, int slices, int64_t M, int64_t Hq, int64_t Hkv, int64_t d, mm355_bf16* qkv,
                                             int64_t ld_qkv, const mm355_bf16* cos_t, const mm355_bf16* sin_t, const int32_t* positions,
                                             mm355_bf16* k_cache, mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, hipStream_t stream);

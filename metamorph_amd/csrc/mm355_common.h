// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of libmm355.so.
// wave = 64 lanes; bf16 is carried as raw 16-bit words (uint16_t / short vectors).
#pragma once

#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>

#include "../../include/mm355.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;     // one MFMA A/B fragment (8 bf16 = 16 B)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;      // one 16x16 MFMA accumulator fragment
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define MM_DEV __device__ __forceinline__

MM_DEV float bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
MM_DEV uint16_t f2bf(float f) {                      // RNE, lowers to v_cvt_pk_bf16_f32 on gfx950
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
// one v_cvt_pk_bf16_f32 (the scalar form costs two conversions, a shift and an or)
typedef float mm_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 mm_bf16x2 __attribute__((ext_vector_type(2)));
MM_DEV uint32_t pack2bf(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(mm_f32x2{lo, hi}, mm_bf16x2));
}
MM_DEV float bflo(uint32_t w) { return __uint_as_float(w << 16); }
MM_DEV float bfhi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
MM_DEV float round_bf(float f) { return bf2f(f2bf(f)); }

// 8 bf16 <-> 8 floats
MM_DEV void unpack8(const u32x4& v, float* f) {
    f[0] = bflo(v.x); f[1] = bfhi(v.x); f[2] = bflo(v.y); f[3] = bfhi(v.y);
    f[4] = bflo(v.z); f[5] = bfhi(v.z); f[6] = bflo(v.w); f[7] = bfhi(v.w);
}
MM_DEV u32x4 pack8(const float* f) {
    u32x4 v;
    v.x = pack2bf(f[0], f[1]); v.y = pack2bf(f[2], f[3]); v.z = pack2bf(f[4], f[5]); v.w = pack2bf(f[6], f[7]);
    return v;
}

// four e4m3 bytes (k .. k+3) -> the packed bf16 pairs (k, k+1) and (k+2, k+3): exact (e4m3 -> fp32 is exact and its upper 16 bits ARE the
// bf16 value).  Shared by the w8 GEMVs (decode_w8.hip) and the w8 GEMM (gemm_w8.hip).
MM_DEV void e4m3x4_to_bf16(uint32_t q, uint32_t& p01, uint32_t& p23) {
    const mm_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, false);
    const mm_f32x2 b = __builtin_amdgcn_cvt_pk_f32_fp8((int)q, true);
    p01 = __builtin_amdgcn_perm(__float_as_uint(a.y), __float_as_uint(a.x), 0x07060302u);
    p23 = __builtin_amdgcn_perm(__float_as_uint(b.y), __float_as_uint(b.x), 0x07060302u);
}

// MXFP4: dword q = eight e2m1 values k .. k+7 (byte b: k + 2b in the low nibble), sc = 2^(S - 127) -> the packed bf16 pairs (k, k+1) ..
// (k+6, k+7): four v_cvt_scalef32_pk_bf16_fp4, exact, the group scale inside the conversion.  Shared by the w4 GEMVs (decode_w4.hip) and
// the w4 GEMM (gemm_w4.hip).
MM_DEV void e2m1x8_to_bf16(uint32_t q, float sc, uint32_t (&p)[4]) {
    p[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 0));
    p[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 1));
    p[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 2));
    p[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, sc, 3));
}
MM_DEV float e8m0_to_f32(uint32_t s) { return __uint_as_float(s << 23); }     // (S in 1 .. 254: a normal fp32)

MM_DEV float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
MM_DEV float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// block-wide sum for blockDim.x = NT (multiple of 64); `red` needs NT/64 floats of LDS.
template <int NT>
MM_DEV float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}
template <int NT>
MM_DEV float block_max(float v, float* red) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) red[w] = v;
    __syncthreads();
    float t = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) t = fmaxf(t, red[i]);
    return t;
}

MM_DEV float gelu_erf_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
MM_DEV float gelu_tanh_f(float x) {
    const float c = 0.79788456080286535588f;
    return 0.5f * x * (1.0f + tanhf(c * (x + 0.044715f * x * x * x)));
}
MM_DEV float gelu_erf_grad(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}
MM_DEV float gelu_tanh_grad(float x) {
    const float c = 0.79788456080286535588f;
    const float u = c * (x + 0.044715f * x * x * x);
    const float t = tanhf(u);
    const float du = c * (1.0f + 3.0f * 0.044715f * x * x);
    return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * du;
}

// ---- THE definitions of the arithmetic a fused kernel shares with the launch sequence it replaces (the tests compare bits): every
// kernel that applies SwiGLU or the forward rotation calls these; the 8-wide loops and the packing stay with the callers.
// SwiGLU forward: bf16(SiLU(g)) * u, the caller rounds the product
MM_DEV float swiglu_f(float g, float u) { return round_bf(g / (1.0f + __expf(-g))) * u; }
// SwiGLU backward: (g, u, dact) -> dg, du and the recomputed act, each rounded by the caller
MM_DEV void swiglu_bwd_f(float g, float u, float dact, float& dg, float& du, float& act) {
    const float sg = 1.0f / (1.0f + __expf(-g));
    const float silu = g * sg;
    act = round_bf(silu) * u;
    du = dact * round_bf(silu);
    dg = dact * u * (sg * (1.0f + g * (1.0f - sg)));
}
// The forward rotation in HF rounding order, bf(bf(x c) + bf(-+ partner s)): x in the first half of a head (partner d/2 above it) takes
// rope_lo, x in the second half (partner d/2 below) rope_hi; the caller rounds the sum
MM_DEV float rope_lo(float x, float partner, float c, float s) { return round_bf(x * c) + round_bf(-partner * s); }
MM_DEV float rope_hi(float x, float partner, float c, float s) { return round_bf(x * c) + round_bf(partner * s); }
// The inverse rotation of a gradient (rope_qk_kernel): dx1 = dy1 c + dy2 s with the second product fused into the sum, dx2 = dy2 c - dy1 s
// with both products rounded -- written out, so that the bits do not hang on what the compiler chooses to contract
MM_DEV float rope_inv_lo(float dy, float partner, float c, float s) {
#pragma clang fp contract(off)
    return fmaf(partner, s, dy * c);
}
MM_DEV float rope_inv_hi(float dy, float partner, float c, float s) {
#pragma clang fp contract(off)
    return dy * c - partner * s;
}

static inline int mm_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MM355_OK : MM355_ELAUNCH;
}
// Dynamic-LDS opt-in of a kernel (> 64 KiB): hipFuncSetAttribute acts on the CURRENT device's copy of the function, so it is done once
// per device (a bit per device ordinal in a per-kernel mask); a process driving several GPUs gets every device configured.
static inline int mm_ensure_dynamic_lds(const void* kernel, int bytes, std::atomic<uint64_t>& done) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MM355_ELAUNCH;
    const uint64_t bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_acquire) & bit)) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return MM355_ELAUNCH;
        done.fetch_or(bit, std::memory_order_release);       // idempotent: a concurrent first call just sets the attribute twice
    }
    return MM355_OK;
}
static inline bool mm_aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

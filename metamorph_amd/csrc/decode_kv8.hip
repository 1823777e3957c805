// Writing an FP8 KV cache (gfx950; its readers: attn_decode.hip, attn_extend.hip, attn_extend_shared.hip).  One cached head-row -- the d
// post-RoPE bf16 values of one KV head of one token -- is stored as d OCP e4m3fn bytes plus ONE fp32 scale:
//   scale = the smallest power of two with amax / scale <= 448 (a head-row of zeros: 1),  q[c] = RNE_e4m3(x[c] / scale)
// x / scale is an exponent shift (exact), nothing saturates, fp32(q[c]) * scale is exact and a bf16 value.  So every reader of the cache can
// be held, bit for bit, to the bf16 kernels on the dequantised rows.
// kv_quant_kernel / rope_kv_append_f8_kernel: one head-row per 16-lane group (8 columns per lane), amax folded across the group.
#include "mm355_common.h"

namespace {

constexpr int NT = 256;

// The 8 columns of one lane of a 16-lane head-row group (lanes beyond d carry zeros) -> their 8 bytes; returns the group's scale.
MM_DEV float quant_headrow8(const float* x, u32x2& q) {
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(x[e]));
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) a = fmaxf(a, __shfl_xor(a, o, 16));
    int ex = 0;
    const float m = frexpf(a, &ex);                          // a = m * 2^ex, m in [0.5, 1): 448 = 0.875 * 2^9
    const int sh = a > 0.f ? ex - 9 + (m > 0.875f ? 1 : 0) : 0;
    float y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = ldexpf(x[e], -sh);
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
    q = u32x2{(uint32_t)w0, (uint32_t)w1};
    return ldexpf(1.f, sh);
}

// src row r, KV head hk -> cache row row0 + r % rows_per_seq of sequence r / rows_per_seq
__global__ __launch_bounds__(NT) void kv_quant_kernel(const uint16_t* __restrict__ src, int64_t ld_src, int64_t n_rows, int64_t rows_per_seq, int Hkv,
                                                      int d, uint8_t* __restrict__ dst, int64_t ld_dst, float* __restrict__ dsc, int64_t ld_sc,
                                                      int64_t bs_dst, int64_t bs_sc, int64_t row0) {
    const int dc = threadIdx.x & 15;
    const int64_t grp = (int64_t)blockIdx.x * (NT / 16) + (threadIdx.x >> 4);
    const bool live = grp < n_rows * Hkv;                    // (uniform over the 16 lanes of a group)
    const int64_t r = live ? grp / Hkv : 0;
    const int hk = live ? (int)(grp % Hkv) : 0;
    const bool on = dc * 8 < d;
    float x[8];
    unpack8(on ? *(const u32x4*)(src + r * ld_src + (int64_t)hk * d + dc * 8) : u32x4{0u, 0u, 0u, 0u}, x);
    u32x2 q;
    const float sc = quant_headrow8(x, q);
    if (!live) return;
    const int64_t seq = r / rows_per_seq, row = row0 + r % rows_per_seq;
    if (on) *(u32x2*)(dst + seq * bs_dst + row * ld_dst + (int64_t)hk * d + dc * 8) = q;
    if (dc == 0) dsc[seq * bs_sc + row * ld_sc + hk] = sc;
}

// rope_kv_append_kernel with an e4m3 cache: blocks [0, nqb) rotate q in place (that kernel's items), the others take one K or V head-row per
// 16-lane group: a lane rotates its own 8 columns (the partner half is a second load), rounds them to bf16 as the bf16 kernel stores them,
// and the group quantises that row.
MM_DEV void rope_kv_append_f8_row(uint16_t* __restrict__ row, int pos, int Hq, int Hkv, int d, const uint16_t* __restrict__ cos_t,
                                  const uint16_t* __restrict__ sin_t, uint8_t* __restrict__ krow, uint8_t* __restrict__ vrow,
                                  float* __restrict__ ksrow, float* __restrict__ vsrow, int nqb, int bx) {
    const int half = d >> 1, vph = half >> 3;
    if (bx < nqb) {
        const int i = bx * NT + threadIdx.x;
        if (i >= Hq * vph) return;
        const int v = i % vph, hd = i / vph;
        uint16_t* p1 = row + (int64_t)hd * d + v * 8;
        uint16_t* p2 = p1 + half;
        float x1[8], x2[8], c[8], sn[8], y1[8], y2[8];
        unpack8(*(const u32x4*)p1, x1);
        unpack8(*(const u32x4*)p2, x2);
        unpack8(*(const u32x4*)(cos_t + (int64_t)pos * d + v * 8), c);
        unpack8(*(const u32x4*)(sin_t + (int64_t)pos * d + v * 8), sn);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            y1[e] = rope_lo(x1[e], x2[e], c[e], sn[e]);
            y2[e] = rope_hi(x2[e], x1[e], c[e], sn[e]);
        }
        *(u32x4*)p1 = pack8(y1);
        *(u32x4*)p2 = pack8(y2);
        return;
    }
    const int dc = threadIdx.x & 15;
    const int grp = (bx - nqb) * (NT / 16) + (threadIdx.x >> 4);      // [0, Hkv): K heads, [Hkv, 2 Hkv): V heads
    const bool live = grp < 2 * Hkv;
    const bool isv = grp >= Hkv;
    const int hk = live ? (isv ? grp - Hkv : grp) : 0;
    const bool on = dc * 8 < d;
    const int c0 = on ? dc * 8 : 0;
    const uint16_t* hp = row + (int64_t)(Hq + (isv && live ? Hkv : 0) + hk) * d;
    float x[8];
    unpack8(*(const u32x4*)(hp + c0), x);
    if (!isv) {
        const bool lo = c0 < half;
        const int v8 = lo ? c0 : c0 - half;
        float xp[8], c[8], sn[8], y[8];
        unpack8(*(const u32x4*)(hp + (lo ? c0 + half : c0 - half)), xp);
        unpack8(*(const u32x4*)(cos_t + (int64_t)pos * d + v8), c);
        unpack8(*(const u32x4*)(sin_t + (int64_t)pos * d + v8), sn);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            y[e] = lo ? rope_lo(x[e], xp[e], c[e], sn[e]) : rope_hi(x[e], xp[e], c[e], sn[e]);
        unpack8(pack8(y), x);                                // the bf16 row the bf16 kernel would have cached
    }
    if (!on) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
    }
    u32x2 q;
    const float sc = quant_headrow8(x, q);
    if (!live) return;
    uint8_t* dst = (isv ? vrow : krow) + (int64_t)hk * d;
    if (on) *(u32x2*)(dst + dc * 8) = q;
    if (dc == 0) (isv ? vsrow : ksrow)[hk] = sc;
}

__global__ __launch_bounds__(NT) void rope_kv_append_f8_kernel(uint16_t* __restrict__ qkv, int64_t ld, int Hq, int Hkv, int d,
                                                               const uint16_t* __restrict__ cos_t, const uint16_t* __restrict__ sin_t,
                                                               const int32_t* __restrict__ positions, uint8_t* __restrict__ kc,
                                                               uint8_t* __restrict__ vc, int64_t ld_kv, int64_t bs_kv, float* __restrict__ ks,
                                                               float* __restrict__ vs, int64_t ld_sc, int64_t bs_sc, int nqb) {
    const int b = blockIdx.y;
    const int pos = positions[b];
    const int64_t ob = (int64_t)b * bs_kv + (int64_t)pos * ld_kv, os = (int64_t)b * bs_sc + (int64_t)pos * ld_sc;
    rope_kv_append_f8_row(qkv + (int64_t)b * ld, pos, Hq, Hkv, d, cos_t, sin_t, kc + ob, vc + ob, ks + os, vs + os, nqb, (int)blockIdx.x);
}

// rope_kv_append_rows_kernel (decode.hip) with an e4m3 cache: row r on grid.x, its q blocks and head-row groups on grid.y
__global__ __launch_bounds__(NT) void rope_kv_append_rows_f8_kernel(uint16_t* __restrict__ qkv, int64_t ld, int Hq, int Hkv, int d,
                                                                    const uint16_t* __restrict__ cos_t, const uint16_t* __restrict__ sin_t,
                                                                    const int32_t* __restrict__ positions, const int32_t* __restrict__ blocks,
                                                                    int n_blocks, int rows_per_block, uint8_t* __restrict__ kc,
                                                                    uint8_t* __restrict__ vc, int64_t ld_kv, int64_t bs_kv, float* __restrict__ ks,
                                                                    float* __restrict__ vs, int64_t ld_sc, int64_t bs_sc, int nqb) {
    const int r = blockIdx.x;
    const int pos = min(max(positions[r], 0), rows_per_block - 1);
    const int blk = min(max(blocks ? blocks[r] : r, 0), n_blocks - 1);
    const int64_t ob = (int64_t)blk * bs_kv + (int64_t)pos * ld_kv, os = (int64_t)blk * bs_sc + (int64_t)pos * ld_sc;
    rope_kv_append_f8_row(qkv + (int64_t)r * ld, pos, Hq, Hkv, d, cos_t, sin_t, kc + ob, vc + ob, ks + os, vs + os, nqb, (int)blockIdx.y);
}

bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

}  // namespace

extern "C" int mm355_kv_quant_f8(const mm355_bf16* src, int64_t ld_src, int64_t n_rows, int64_t rows_per_seq, int64_t Hkv, int64_t d,
                                 uint8_t* dst_bytes, int64_t ld_dst_bytes, float* dst_scale, int64_t ld_scale, int64_t batch_stride_bytes,
                                 int64_t batch_stride_scale, int64_t row0, int fmt, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !src || !dst_bytes || !dst_scale || n_rows <= 0 || rows_per_seq <= 0 || Hkv <= 0 || d <= 0 || row0 < 0)
        return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if (!mm_aligned16(src) || (ld_src & 7) || !aligned8(dst_bytes) || (ld_dst_bytes & 7) || (batch_stride_bytes & 7) || (((uintptr_t)dst_scale) & 3u) ||
        ld_src < Hkv * d || ld_dst_bytes < Hkv * d || ld_scale < Hkv)
        return MM355_EINVAL;
    const int64_t blocks = (n_rows * Hkv + NT / 16 - 1) / (NT / 16);
    if (blocks > 0x7fffffff || Hkv > 0x7fffffff) return MM355_EINVAL;
    hipLaunchKernelGGL(kv_quant_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, src, ld_src, n_rows, rows_per_seq, (int)Hkv, (int)d,
                       dst_bytes, ld_dst_bytes, dst_scale, ld_scale, batch_stride_bytes, batch_stride_scale, row0);
    return mm_launch_status();
}

extern "C" int mm355_rope_kv_append_f8(mm355_bf16* qkv, int64_t ld, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, const mm355_bf16* cos_t,
                                       const mm355_bf16* sin_t, const int32_t* positions, uint8_t* k_cache, uint8_t* v_cache, int64_t ld_kv_bytes,
                                       int64_t batch_stride_kv_bytes, float* k_scale, float* v_scale, int64_t ld_scale, int64_t batch_stride_scale,
                                       int fmt, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || !k_scale || !v_scale || B <= 0 || Hq <= 0 ||
        Hkv <= 0 || d <= 0 || B > 65535)
        return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if (d & 15) return MM355_EINVAL;                         // (rotation partners in 16-byte vectors, as mm355_rope_kv_append)
    if ((ld & 7) || !mm_aligned16(qkv) || !mm_aligned16(cos_t) || !mm_aligned16(sin_t) || !aligned8(k_cache) || !aligned8(v_cache) ||
        (ld_kv_bytes & 7) || (batch_stride_kv_bytes & 7) || ((((uintptr_t)k_scale) | ((uintptr_t)v_scale)) & 3u) || ld_kv_bytes < Hkv * d ||
        ld_scale < Hkv)
        return MM355_EINVAL;
    const int nqb = (int)((Hq * (d / 16) + NT - 1) / NT);
    const int nkb = (int)((2 * Hkv + NT / 16 - 1) / (NT / 16));
    hipLaunchKernelGGL(rope_kv_append_f8_kernel, dim3((unsigned)(nqb + nkb), (unsigned)B), dim3(NT), 0, (hipStream_t)stream, qkv, ld, (int)Hq,
                       (int)Hkv, (int)d, cos_t, sin_t, positions, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale,
                       batch_stride_scale, nqb);
    return mm_launch_status();
}

extern "C" int mm355_rope_kv_append_rows_f8(mm355_bf16* qkv, int64_t ld, int64_t R, int64_t Hq, int64_t Hkv, int64_t d, const mm355_bf16* cos_t,
                                            const mm355_bf16* sin_t, const int32_t* positions, const int32_t* blocks, int64_t n_blocks,
                                            int64_t rows_per_block, uint8_t* k_cache, uint8_t* v_cache, int64_t ld_kv_bytes,
                                            int64_t batch_stride_kv_bytes, float* k_scale, float* v_scale, int64_t ld_scale,
                                            int64_t batch_stride_scale, int fmt, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !qkv || !cos_t || !sin_t || !positions || !k_cache || !v_cache || !k_scale || !v_scale || R <= 0 || Hq <= 0 ||
        Hkv <= 0 || d <= 0 || R > 0x7fffffffll || n_blocks < 1 || rows_per_block < 1 || n_blocks > 0x7fffffffll || rows_per_block > 0x7fffffffll ||
        (!blocks && n_blocks < R))
        return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if (d & 15) return MM355_EINVAL;
    if ((ld & 7) || !mm_aligned16(qkv) || !mm_aligned16(cos_t) || !mm_aligned16(sin_t) || !aligned8(k_cache) || !aligned8(v_cache) ||
        (ld_kv_bytes & 7) || (batch_stride_kv_bytes & 7) || ((((uintptr_t)k_scale) | ((uintptr_t)v_scale)) & 3u) || ld_kv_bytes < Hkv * d ||
        ld_scale < Hkv)
        return MM355_EINVAL;
    const int nqb = (int)((Hq * (d / 16) + NT - 1) / NT);
    const int nkb = (int)((2 * Hkv + NT / 16 - 1) / (NT / 16));
    hipLaunchKernelGGL(rope_kv_append_rows_f8_kernel, dim3((unsigned)R, (unsigned)(nqb + nkb)), dim3(NT), 0, (hipStream_t)stream, qkv, ld, (int)Hq,
                       (int)Hkv, (int)d, cos_t, sin_t, positions, blocks, (int)n_blocks, (int)rows_per_block, k_cache, v_cache, ld_kv_bytes,
                       batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, nqb);
    return mm_launch_status();
}

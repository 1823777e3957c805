// The GEMM argument block and the fused store of eight adjacent output columns (bias / GELU / residual / accumulate / fp32 or bf16
// output) with the accumulator epilogue around it, shared by every kernel of gemm_bf16.hip and the quantised-weight skeleton of gemm_wq.h
// (gemm_w8.hip, gemm_w4.hip) so that all of them round exactly the same way; and the workgroup -> tile map they share.
#pragma once
#include "mm355_common.h"

namespace {

struct GemmArgs {
    const uint16_t* A;
    const uint16_t* B;
    void* C;
    const uint16_t* bias;
    const uint16_t* res;
    int64_t lda, ldb, ldc, ldr, res_mod;
    int M, N, K;
    uint32_t flags;
    int ntm, ntn;
    int gm;                                                  // raster group height in tiles (ping-pong kernel)
    uint16_t* aux0;                                          // fused SwiGLU-backward epilogue: actT [I][ld_aux]
    uint16_t* aux1;                                          //                                 dguT [2 I][ld_aux]
    int64_t ld_aux;
    int kslice;                                              // split-K (gemm_nt_kernel only): K elements per blockIdx.y slice, 0 = off; C is then the
};                                                           // fp32 partial buffer [slices][M][ldc]

// workgroup `bid` of a grid of ntm x ntn tiles -> its tile (tm, tn).  Workgroups go to the eight XCDs round-robin: each XCD gets one
// contiguous range of the logical order, and that order walks the tiles in groups of GM tile rows, down a group's column first, so that
// the workgroups resident together on an XCD share A and B panels in its L2.
MM_DEV void gemm_tile_map(const int ntm, const int ntn, const int GM, const int bid, int& tm, int& tn) {
    const int total = ntm * ntn;
    const int q8 = total >> 3, r8 = total & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int logical = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + idx;
    const int gsize = GM * ntn;
    const int grp = logical / gsize;
    const int first_m = grp * GM;
    const int gm = min(ntm - first_m, GM);
    const int in_g = logical - grp * gsize;
    tm = first_m + in_g % gm;
    tn = in_g / gm;
}

// ragged-edge epilogue (N tail or unaligned leading dimensions): one element at a time, kept out of line
// so the unrolled fast path stays small.
// (arguments by value: taking the address of the kernel-argument struct would push it into scratch memory)
__device__ __attribute__((noinline)) void epi_scalar(void* C, int64_t ldc, const uint16_t* bias, const uint16_t* res, int64_t ldr,
                                                     uint32_t fl, int N, int grow, int c, int64_t rr, float v0, float v1,
                                                     float v2, float v3, float v4, float v5, float v6, float v7) {
    const float v[8] = {v0, v1, v2, v3, v4, v5, v6, v7};
    for (int e = 0; e < 8; ++e) {
        const int ce = c + e;
        if (ce >= N) break;
        float x = v[e];
        if (fl & MM355_GEMM_BIAS) x += bf2f(bias[ce]);
        if (fl & MM355_GEMM_GELU_ERF) x = gelu_erf_f(x);
        else if (fl & MM355_GEMM_GELU_TANH) x = gelu_tanh_f(x);
        if (fl & MM355_GEMM_RESIDUAL) x += bf2f(res[rr * ldr + ce]);
        if (fl & MM355_GEMM_OUT_F32) {
            float* p = (float*)C + (int64_t)grow * ldc + ce;
            if (fl & MM355_GEMM_ACCUMULATE) x += *p;
            *p = x;
        } else {
            uint16_t* p = (uint16_t*)C + (int64_t)grow * ldc + ce;
            if (fl & MM355_GEMM_ACCUMULATE) x += bf2f(*p);
            *p = f2bf(x);
        }
    }
}

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

// eight adjacent columns c .. c + 7 of output row `grow` (rr = residual row) from fp32 accumulators v[0..7]; c < N
MM_DEV void epi_store8(const GemmArgs& a, const uint32_t fl, const bool vec_ok, const int grow, const int64_t rr, const int c, float (&v)[8]) {
    const int N = a.N;
    uint16_t* Cb = (uint16_t*)a.C;
    float* Cf = (float*)a.C;
    const bool full = (c + 8 <= N) && vec_ok;
    if (full) {
        if (fl & MM355_GEMM_BIAS) {
            float b[8];
            unpack8(*(const u32x4*)(a.bias + c), b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
        }
        if (fl & MM355_GEMM_GELU_ERF) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = gelu_erf_f(v[e]);
        } else if (fl & MM355_GEMM_GELU_TANH) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = gelu_tanh_f(v[e]);
        }
        if (fl & MM355_GEMM_RESIDUAL) {
            float b[8];
            unpack8(*(const u32x4*)(a.res + rr * a.ldr + c), b);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += b[e];
        }
        if (fl & MM355_GEMM_OUT_F32) {
            float* p = Cf + (int64_t)grow * a.ldc + c;
            if (fl & MM355_GEMM_ACCUMULATE) {
                const f32x4 o0 = *(const f32x4*)p, o1 = *(const f32x4*)(p + 4);
                v[0] += o0.x; v[1] += o0.y; v[2] += o0.z; v[3] += o0.w;
                v[4] += o1.x; v[5] += o1.y; v[6] += o1.z; v[7] += o1.w;
            }
            *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
            *(f32x4*)(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
        } else {
            uint16_t* p = Cb + (int64_t)grow * a.ldc + c;
            if (fl & MM355_GEMM_ACCUMULATE) {
                float b[8];
                unpack8(*(const u32x4*)p, b);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += b[e];
            }
            *(u32x4*)p = pack8(v);
        }
    } else {
        epi_scalar(a.C, a.ldc, a.bias, a.res, a.ldr, fl, N, grow, c, rr, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    }
}

// Shared epilogue (every gemm_nt_kernel form and gemm_wq_kernel in gemm_wq.h): accumulators -> wave-private LDS slab -> row-contiguous 16-B stores with the fused epilogue.
template <int TM, int TN, int FM, int FN>
MM_DEV void gemm_epilogue(f32x4 (&acc)[FM][FN], const GemmArgs& a, unsigned char* smem, int m0, int n0, int wm, int wn, int wave, int lane) {
    const int fr = lane & 15, fq = lane >> 4;
    const int M = a.M, N = a.N;
    constexpr int CPL = TN / 4;                          // columns handled by one lane per row
    float* stg = (float*)smem + wave * (16 * TN);
    const uint32_t fl = a.flags;
    const int row_l = lane >> 2, col_l = (lane & 3) * CPL;
    uint16_t* Cb = (uint16_t*)a.C;
    float* Cf = (float*)a.C;
    const bool vec_ok = ((a.ldc & 7) == 0) && (!(fl & MM355_GEMM_RESIDUAL) || (a.ldr & 7) == 0);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
        // the staging slab is private to this wave and the LDS executes one wave's instructions in order: a wave-level
        // fence (no s_barrier) is all the write -> read -> next write hand-over needs; the caller has already made sure
        // (block barrier) that nobody still reads the tile data this slab overlays
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) stg[(fq * 4 + r) * TN + j * 16 + fr] = acc[i][j][r];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int grow = m0 + wm * TM + i * 16 + row_l;
        if (grow < M) {
            const int64_t rr = (fl & MM355_GEMM_RESIDUAL) ? (a.res_mod > 0 ? (int64_t)(grow % a.res_mod) : (int64_t)grow) : 0;
#pragma unroll
            for (int j = 0; j < CPL / 8; ++j) {
                const int c = n0 + wn * TN + col_l + j * 8;
                if (c >= N) continue;
                float v[8];
                const f32x4 s0 = *(const f32x4*)(stg + row_l * TN + col_l + j * 8);
                const f32x4 s1 = *(const f32x4*)(stg + row_l * TN + col_l + j * 8 + 4);
                v[0] = s0.x; v[1] = s0.y; v[2] = s0.z; v[3] = s0.w;
                v[4] = s1.x; v[5] = s1.y; v[6] = s1.z; v[7] = s1.w;
                epi_store8(a, fl, vec_ok, grow, rr, c, v);
            }
        }
    }
}

}  // namespace

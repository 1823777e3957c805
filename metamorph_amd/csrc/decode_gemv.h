// What the decode GEMVs share (decode.hip: bf16 weights; decode_w8.hip: e4m3 bytes + a scale per row; decode_w4.hip: MXFP4 nibbles + a
// scale byte per 32 columns): the four weight rows of a unit in each mode and the epilogues, templated on the kernel's operand struct (A:
// WqArgs below, GemvArgs in decode.hip), and the operands of the quantised kernels.  The files differ in how a 16-byte load becomes packed
// bf16 pairs and in where the scale enters; everything behind the sum is this header.
#pragma once

#include "mm355_common.h"

namespace {

constexpr int NT = 256;
constexpr uint32_t OOB = 0xf0000000u;                        // or-ed into a buffer offset: beyond num_records, the load returns zeros

struct WqArgs {
    const uint16_t* x; int64_t ldx;
    const uint8_t* W; int64_t ldw;                           // bytes
    const float* scale;                                      // w8: one fp32 scale per weight row
    const uint8_t* S; int64_t lds;                           // w4: one e8m0 scale byte per 32 columns, row stride in bytes
    int M, N, K;                                             // N = weight rows
    const uint16_t* norm_w; float eps;                       // PRENORM
    void* y; int64_t ldy;                                    // MODE 0
    const uint16_t* bias; const uint16_t* res; int64_t ldr; uint32_t flags;
    uint16_t* out; int64_t ld_out;                           // MODE 1: act [M][I]; MODE 2: qkv row buffer [M][N]
    int I;                                                   // MODE 1
    int Hq, Hkv, d;                                          // MODE 2
    const uint16_t* cos_t; const uint16_t* sin_t; const int32_t* positions;
    uint16_t* kc; uint16_t* vc; int64_t ld_kv, bs_kv;
    int ks;                                                  // MFMA form: waves that share one group of 16 weight rows (1, 4)
};

// the four weight rows of a unit: plain = 4u .. 4u+3; SwiGLU = gate rows c, c+1 and up rows I+c, I+c+1; RoPE = the
// rotation partners j, j+1, j+d/2, j+1+d/2 of one head (v rows: four neighbours)
template <int MODE, class A>
MM_DEV void unit_rows(const A& a, int unit, int (&rows)[4]) {
    if constexpr (MODE == 0) {
        rows[0] = unit * 4; rows[1] = rows[0] + 1; rows[2] = rows[0] + 2; rows[3] = rows[0] + 3;
    } else if constexpr (MODE == 1) {
        const int c = unit * 2;
        rows[0] = c; rows[1] = c + 1; rows[2] = a.I + c; rows[3] = a.I + c + 1;
    } else {
        const int upd = a.d / 4, nrot = (a.Hq + a.Hkv) * upd;
        if (unit < nrot) {
            const int hd = unit / upd, j = (unit % upd) * 2;
            rows[0] = hd * a.d + j; rows[1] = rows[0] + 1; rows[2] = rows[0] + a.d / 2; rows[3] = rows[2] + 1;
        } else {
            const int b0 = (a.Hq + a.Hkv) * a.d + (unit - nrot) * 4;
            rows[0] = b0; rows[1] = b0 + 1; rows[2] = b0 + 2; rows[3] = b0 + 3;
        }
    }
}
template <int MODE, class A>
MM_DEV bool unit_live(const A& a, const int (&rows)[4]) {
    if constexpr (MODE == 0) return rows[0] < a.N;
    else if constexpr (MODE == 1) return rows[1] < a.I;
    else return rows[3] < a.N;
}

// MODE 0: output (m, n) of the finished sum v (w8: scale[n] * sum): + bias, GELU, + residual, fp32 or bf16
template <class A>
MM_DEV void plain_store(const A& a, int m, int n, float v) {
    const uint32_t flags = a.flags;
    if (flags & MM355_GEMM_BIAS) v += bf2f(a.bias[n]);
    if (flags & MM355_GEMM_GELU_ERF) v = gelu_erf_f(v);
    if (flags & MM355_GEMM_GELU_TANH) v = gelu_tanh_f(v);
    if (flags & MM355_GEMM_RESIDUAL) v += bf2f(a.res[(int64_t)m * a.ldr + n]);
    if (flags & MM355_GEMM_OUT_F32) ((float*)a.y)[(int64_t)m * a.ldy + n] = v;
    else ((uint16_t*)a.y)[(int64_t)m * a.ldy + n] = f2bf(v);
}

// MODE 1 / 2: the four outputs of one unit for x row m, already rounded to bf16 (what the unfused GEMV stores), through swiglu_f /
// rope_lo and rope_hi (mm355_common.h) as swiglu_fwd_kernel / rope_kv_append_kernel would take them
template <int MODE, class A>
MM_DEV void fused_store(const A& a, const int (&rows)[4], int m, const float (&v4)[4]) {
    if constexpr (MODE == 1) {
        float o[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) o[e] = swiglu_f(v4[e], v4[2 + e]);
        *(uint32_t*)(a.out + (int64_t)m * a.ld_out + rows[0]) = pack2bf(o[0], o[1]);
    } else {
        const int nqk = (a.Hq + a.Hkv) * a.d;
        const int pos = a.positions[m];
        if (rows[0] < nqk) {
            const int hd = rows[0] / a.d, j = rows[0] % a.d;
            float y1[2], y2[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float c = bf2f(a.cos_t[(int64_t)pos * a.d + j + e]), sn = bf2f(a.sin_t[(int64_t)pos * a.d + j + e]);
                y1[e] = rope_lo(v4[e], v4[2 + e], c, sn);
                y2[e] = rope_hi(v4[2 + e], v4[e], c, sn);
            }
            uint16_t* dst = hd < a.Hq ? a.out + (int64_t)m * a.ld_out + rows[0]
                                      : a.kc + (int64_t)m * a.bs_kv + (int64_t)pos * a.ld_kv + (int64_t)(hd - a.Hq) * a.d + j;
            *(uint32_t*)dst = pack2bf(y1[0], y1[1]);
            *(uint32_t*)(dst + a.d / 2) = pack2bf(y2[0], y2[1]);
        } else {
            uint16_t* dst = a.vc + (int64_t)m * a.bs_kv + (int64_t)pos * a.ld_kv + (rows[0] - nqk);
            *(u32x2*)dst = u32x2{pack2bf(v4[0], v4[1]), pack2bf(v4[2], v4[3])};
        }
    }
}

}  // namespace

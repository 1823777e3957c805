// Cached decode over an FP8 KV cache (gfx950).  One cached head-row -- the d post-RoPE bf16 values of one KV head of one token -- is stored as
// d OCP e4m3fn bytes plus ONE fp32 scale:
//   scale = the smallest power of two with amax / scale <= 448 (a head-row of zeros: 1),  q[c] = RNE_e4m3(x[c] / scale)
// x / scale is an exponent shift (exact), nothing saturates, fp32(q[c]) * scale is exact and a bf16 value.  So every reader of the cache can
// be held, bit for bit, to the bf16 kernels of decode.hip on the dequantised rows:
//   * kv_quant_kernel / rope_kv_append_f8_kernel: one head-row per 16-lane group (8 columns per lane), amax folded across the group;
//   * attn_decode_f8_kernel: attn_decode_wide_kernel with 8-byte loads per lane, the same key-to-thread map, folds and merge; the scales
//     are applied once per key (score: after the 16-lane fold; value: on the probability), never per element.
#include "mm355_common.h"

namespace {

constexpr int NT = 256;
constexpr int CH = 256;                                      // keys per sub-block (decode.hip)

MM_DEV void unpack8_f8(const u32x2& v, float* f) {
    const mm_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
    const mm_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = e.x; f[7] = e.y;
}

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
__global__ __launch_bounds__(NT) void rope_kv_append_f8_kernel(uint16_t* __restrict__ qkv, int64_t ld, int Hq, int Hkv, int d,
                                                               const uint16_t* __restrict__ cos_t, const uint16_t* __restrict__ sin_t,
                                                               const int32_t* __restrict__ positions, uint8_t* __restrict__ kc,
                                                               uint8_t* __restrict__ vc, int64_t ld_kv, int64_t bs_kv, float* __restrict__ ks,
                                                               float* __restrict__ vs, int64_t ld_sc, int64_t bs_sc, int nqb) {
    const int b = blockIdx.y;
    const int pos = positions[b];
    const int half = d >> 1, vph = half >> 3;
    uint16_t* row = qkv + (int64_t)b * ld;
    if ((int)blockIdx.x < nqb) {
        const int i = blockIdx.x * NT + threadIdx.x;
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
            y1[e] = round_bf(x1[e] * c[e]) + round_bf(-x2[e] * sn[e]);
            y2[e] = round_bf(x2[e] * c[e]) + round_bf(x1[e] * sn[e]);
        }
        *(u32x4*)p1 = pack8(y1);
        *(u32x4*)p2 = pack8(y2);
        return;
    }
    const int dc = threadIdx.x & 15;
    const int grp = ((int)blockIdx.x - nqb) * (NT / 16) + (threadIdx.x >> 4);      // [0, Hkv): K heads, [Hkv, 2 Hkv): V heads
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
            y[e] = lo ? round_bf(x[e] * c[e]) + round_bf(-xp[e] * sn[e]) : round_bf(x[e] * c[e]) + round_bf(xp[e] * sn[e]);
        unpack8(pack8(y), x);                                // the bf16 row the bf16 kernel would have cached
    }
    if (!on) {
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.f;
    }
    u32x2 q;
    const float sc = quant_headrow8(x, q);
    if (!live) return;
    uint8_t* dst = (isv ? vc : kc) + (int64_t)b * bs_kv + (int64_t)pos * ld_kv + (int64_t)hk * d;
    if (on) *(u32x2*)(dst + dc * 8) = q;
    if (dc == 0) (isv ? vs : ks)[(int64_t)b * bs_sc + (int64_t)pos * ld_sc + hk] = sc;
}

// attn_decode_wide_kernel (decode.hip) over e4m3 rows: the same sub-blocks, key-to-thread maps, DPP / shuffle folds, LDS records, merge and
// arrival counters.  A lane's 8 columns are one 8-byte load; the thread that owns key t in the softmax phase reads that key's two scales
// and applies them there: the score it picks up from LDS times k_scale, the probability it puts back times v_scale.  With power-of-two
// scales every fp32 value of the bf16 kernel on the dequantised cache is reproduced exactly.
template <int G>
__global__ __launch_bounds__(1024) void attn_decode_f8_kernel(const uint16_t* __restrict__ q, int64_t ld_q, const uint8_t* __restrict__ kc,
                                                              const uint8_t* __restrict__ vc, int64_t ld_kv, int64_t bs_kv,
                                                              const float* __restrict__ ksc, const float* __restrict__ vsc, int64_t ld_sc,
                                                              int64_t bs_sc, const int32_t* __restrict__ kv_lens, float* __restrict__ ws,
                                                              int ngroup, int Hq, int Hkv, int d, float scale, uint16_t* __restrict__ o,
                                                              int64_t ld_o, int* __restrict__ counters, int kvdiv) {
    constexpr int SB = 4;
    constexpr int NB = G >= 8 ? 2 : (G >= 4 ? 4 : 8);
    constexpr int NBK = G == 1 ? 16 : NB;
    constexpr int VPRE = G == 1 ? 16 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    float (*sp)[G][CH] = (float (*)[G][CH])(lds_f);                             // [SB][G][CH] scores, then probabilities * v_scale
    float (*redm)[G][4] = (float (*)[G][4])(lds_f + SB * G * CH);               // [SB][G][4] per-wave maxima
    float (*reds)[G][4] = (float (*)[G][4])(lds_f + SB * G * CH + SB * G * 4);
    float (*so)[G][128] = (float (*)[G][128])(lds_f + SB * G * CH + 2 * SB * G * 4);   // [SB * 4 waves][G][128]
    __shared__ int last_s;
    const int grp = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, sb = tid >> 8, t = tid & 255, lane = tid & 63, wave = t >> 6;
    const int kv_len = kv_lens[b];
    const int ngr_live = (kv_len + SB * CH - 1) / (SB * CH);
    const int rec = d + 2;
    float* wrec = ws + (((int64_t)b * Hq + hk * G) * ngroup + grp) * rec;
    const int k0 = (grp * SB + sb) * CH;
    const bool active = k0 < kv_len;
    const int dc8_t = ((t & 15) * 8 < d) ? (t & 15) * 8 : 0;
    const int hkv = hk / kvdiv;
    const uint8_t* const kbase = kc + (int64_t)b * bs_kv + (int64_t)hkv * d + dc8_t;
    const uint8_t* const vbase = vc + (int64_t)b * bs_kv + (int64_t)hkv * d + dc8_t;
    if (grp * SB * CH < kv_len) {
        float ksk = 1.f, vsk = 1.f;                          // the scales of key k0 + t (clamped as the rows are)
        if (active) {
            const int64_t so_ = (int64_t)b * bs_sc + (int64_t)min(k0 + t, kv_len - 1) * ld_sc + hkv;
            ksk = ksc[so_];
            vsk = vsc[so_];
        }
        if (active) {
            const int dc = lane & 15, kq = lane >> 4;
            float qreg[G][8];
            {
                const bool qvec = ((((uintptr_t)q) | ((uintptr_t)ld_q * 2u)) & 15u) == 0;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint16_t* qp = q + (int64_t)b * ld_q + (int64_t)(hk * G + g) * d + dc8_t;
                    u32x4 qh;
                    if (qvec) {
                        qh = *(const u32x4*)qp;
                    } else {
                        uint32_t w[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) w[e] = (uint32_t)qp[2 * e] | ((uint32_t)qp[2 * e + 1] << 16);
                        qh = u32x4{w[0], w[1], w[2], w[3]};
                    }
                    float qf[8];
                    unpack8(qh, qf);
#pragma unroll
                    for (int e = 0; e < 8; ++e) qreg[g][e] = (dc * 8 < d) ? qf[e] * scale : 0.f;
                }
            }
#pragma unroll 1
            for (int h = 0; h < 16 / NBK; ++h) {
                u32x2 kraw[NBK];
#pragma unroll
                for (int i = 0; i < NBK; ++i) {
                    const int kk = k0 + wave * 64 + (h * NBK + i) * 4 + kq;
                    kraw[i] = *(const u32x2*)(kbase + (int64_t)min(kk, kv_len - 1) * ld_kv);
                }
#pragma unroll
                for (int i = 0; i < NBK; ++i) {
                    const int kl = wave * 64 + (h * NBK + i) * 4 + kq;
                    const int kk = k0 + kl;
                    float kf[8];
                    unpack8_f8(kraw[i], kf);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        float v = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v = fmaf(kf[e], qreg[g][e], v);
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
                        if (dc == 15) sp[sb][g][kl] = (kk < kv_len) ? v : -INFINITY;
                    }
                }
            }
        }
        u32x2 vpre[VPRE ? VPRE : 1];
        if constexpr (VPRE > 0) {
            if (active) {
#pragma unroll
                for (int i = 0; i < VPRE; ++i) vpre[i] = *(const u32x2*)(vbase + (int64_t)min(k0 + (t >> 4) + i * 16, kv_len - 1) * ld_kv);
            }
        }
        __syncthreads();
        const int key = k0 + t;
        float sc[G];
        if (active) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sc[g] = sp[sb][g][t] * ksk;                  // k_scale[key]: once per key and head (-inf stays -inf)
                const float w = wave_max(sc[g]);
                if (lane == 0) redm[sb][g][wave] = w;
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float mxg = fmaxf(fmaxf(redm[sb][g][0], redm[sb][g][1]), fmaxf(redm[sb][g][2], redm[sb][g][3]));
                const float p = (key < kv_len) ? __expf(sc[g] - mxg) : 0.f;
                sp[sb][g][t] = p * vsk;                       // v_scale[key] rides on the probability; l sums the bare p
                const float w = wave_sum(p);
                if (lane == 0) reds[sb][g][wave] = w;
            }
        }
        __syncthreads();
        if (active) {
            const int dc = t & 15, kg = t >> 4;
            float acc[G][8];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
            const int kend = min(CH, kv_len - k0);
            auto pv = [&](const u32x2& vr, int kk) {
                float vf[8];
                unpack8_f8(vr, vf);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const float p = (kk < kend) ? sp[sb][g][kk] : 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, vf[e], acc[g][e]);
                }
            };
            if constexpr (VPRE > 0) {
#pragma unroll
                for (int i = 0; i < VPRE; ++i) pv(vpre[i], kg + i * 16);
            }
            constexpr int NBV = (16 - VPRE) < NB ? (16 - VPRE ? 16 - VPRE : 1) : NB;
#pragma unroll 1
            for (int r0 = VPRE; r0 < 16; r0 += NBV) {
                u32x2 vraw[NBV];
#pragma unroll
                for (int i = 0; i < NBV; ++i) vraw[i] = *(const u32x2*)(vbase + (int64_t)min(k0 + kg + (r0 + i) * 16, kv_len - 1) * ld_kv);
#pragma unroll
                for (int i = 0; i < NBV; ++i) pv(vraw[i], kg + (r0 + i) * 16);
            }
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = acc[g][e];
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lane < 16 && dc * 8 < d) so[sb * 4 + wave][g][dc * 8 + e] = v;
                }
        }
        __syncthreads();
        for (int i = tid; i < G * d; i += 1024) {
            const int g = i / d, c = i % d;
            float M4[SB], Mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const bool on = (grp * SB + u) * CH < kv_len;
                M4[u] = on ? fmaxf(fmaxf(redm[u][g][0], redm[u][g][1]), fmaxf(redm[u][g][2], redm[u][g][3])) : -INFINITY;
                Mx = fmaxf(Mx, M4[u]);
            }
            float l = 0.f, acc1 = 0.f;
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                if (M4[u] == -INFINITY) continue;
                const float f = __expf(M4[u] - Mx);
                l += f * ((reds[u][g][0] + reds[u][g][1]) + (reds[u][g][2] + reds[u][g][3]));
                acc1 += f * ((so[u * 4 + 0][g][c] + so[u * 4 + 1][g][c]) + (so[u * 4 + 2][g][c] + so[u * 4 + 3][g][c]));
            }
            if (ngr_live == 1) {
                o[(int64_t)b * ld_o + (int64_t)(hk * G + g) * d + c] = f2bf(l > 0.f ? acc1 / l : 0.f);
            } else {
                float* w = wrec + (int64_t)g * ngroup * rec;
                w[2 + c] = acc1;
                if (c == 0) { w[0] = Mx; w[1] = l; }
            }
        }
    } else if (ngr_live > 1 && tid < G) {
        float* w = wrec + (int64_t)tid * ngroup * rec;
        w[0] = -INFINITY; w[1] = 0.f;
    }
    if (ngr_live == 0 && grp == 0) {                          // an empty cache: a zero row
        for (int i = tid; i < G * d; i += 1024) o[(int64_t)b * ld_o + (int64_t)(hk * G + i / d) * d + i % d] = 0;
    }
    if (ngr_live <= 1) return;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int prev = atomicAdd(&counters[b * Hkv + hk], 1);
        last_s = prev == ngroup - 1;
        if (last_s) counters[b * Hkv + hk] = 0;              // ready for the next launch (graph replay)
    }
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    for (int i = tid; i < G * d; i += 1024) {
        const int g = i / d, c = i % d;
        const float* w = ws + (((int64_t)b * Hq + hk * G + g) * ngroup) * rec;
        float Mx = -INFINITY;
        for (int u = 0; u < ngroup; ++u) Mx = fmaxf(Mx, __builtin_nontemporal_load(w + (int64_t)u * rec));
        float l = 0.f, acc1 = 0.f;
        for (int u = 0; u < ngroup; ++u) {
            const float mm = __builtin_nontemporal_load(w + (int64_t)u * rec);
            if (mm == -INFINITY) continue;
            const float f = __expf(mm - Mx);
            l += f * __builtin_nontemporal_load(w + (int64_t)u * rec + 1);
            acc1 += f * __builtin_nontemporal_load(w + (int64_t)u * rec + 2 + c);
        }
        o[(int64_t)b * ld_o + (int64_t)(hk * G + g) * d + c] = f2bf(l > 0.f ? acc1 / l : 0.f);
    }
}

struct F8Args {
    const uint16_t* q; int64_t ld_q;
    const uint8_t* kc; const uint8_t* vc; int64_t ld_kv, bs_kv;
    const float* ks; const float* vs; int64_t ld_sc, bs_sc;
    const int32_t* kv_lens; float* ws; int* counters;
    int B, Hq, d; float scale; uint16_t* o; int64_t ld_o;
};

// G = query heads per workgroup; Hgrp = Hq / G workgroups per sample and key group, each reading cache head (its index) / kvdiv
template <int G>
int launch_f8(const F8Args& a, int ngroup, int Hgrp, int kvdiv, hipStream_t s) {
    constexpr int LDS = (4 * G * CH + 2 * 4 * G * 4 + 16 * G * 128) * 4;
    static std::atomic<uint64_t> lds_ok{0};
    if (LDS > 65536 && mm_ensure_dynamic_lds((const void*)attn_decode_f8_kernel<G>, LDS, lds_ok) != MM355_OK) return MM355_ELAUNCH;
    hipLaunchKernelGGL(attn_decode_f8_kernel<G>, dim3((unsigned)ngroup, (unsigned)Hgrp, (unsigned)a.B), dim3(1024), LDS, s, a.q, a.ld_q, a.kc, a.vc,
                       a.ld_kv, a.bs_kv, a.ks, a.vs, a.ld_sc, a.bs_sc, a.kv_lens, a.ws, ngroup, a.Hq, Hgrp, a.d, a.scale, a.o, a.ld_o, a.counters,
                       kvdiv);
    return mm_launch_status();
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

static int attn_decode_f8_impl(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                               int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                               int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                               int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !q || !k_cache || !v_cache || !k_scale || !v_scale || !kv_lens || !o || !workspace || B <= 0 || Hq <= 0 ||
        Hkv <= 0 || (Hq % Hkv) || max_kv_len <= 0 || d <= 0)
        return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if ((ld_kv_bytes & 7) || (batch_stride_kv_bytes & 7) || !aligned8(k_cache) || !aligned8(v_cache) ||
        ((((uintptr_t)k_scale) | ((uintptr_t)v_scale)) & 3u) || ld_kv_bytes < Hkv * d || ld_scale < Hkv)
        return MM355_EINVAL;
    if (B > 65535 || Hkv > 65535) return MM355_EINVAL;
    if (variant != 0 && variant != 2) return MM355_EINVAL;   // the forms of mm355_attn_decode_variant that share the wide kernel
    const int G0 = (int)(Hq / Hkv);
    const int64_t cf = (B * Hq + 3) & ~(int64_t)3;            // the arrival counters at the start of the workspace (mm355_attn_decode_ws_floats)
    F8Args a = {q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, kv_lens,
                workspace + cf, (int*)workspace, (int)B, (int)Hq, (int)d, scale, o, ld_o};
    hipStream_t s = (hipStream_t)stream;
    if (variant == 0 && max_kv_len <= 4 * CH && (G0 == 2 || G0 == 4 || G0 == 8) && B * Hq <= 512) {   // mm355_attn_decode's spread of the GQA group
        const int gw = (B * Hq <= 64 || G0 == 2) ? 1 : 2;
        if (gw == 1) return launch_f8<1>(a, 1, (int)Hq, G0, s);
        return launch_f8<2>(a, 1, (int)(Hq / 2), G0 / 2, s);
    }
    const int ngroup = (int)(((max_kv_len + CH - 1) / CH + 3) / 4);
    switch (G0) {
        case 1: return launch_f8<1>(a, ngroup, (int)Hkv, 1, s);
        case 2: return launch_f8<2>(a, ngroup, (int)Hkv, 1, s);
        case 4: return launch_f8<4>(a, ngroup, (int)Hkv, 1, s);
        case 8: return launch_f8<8>(a, ngroup, (int)Hkv, 1, s);
        default: return MM355_EUNSUPPORTED;                  // GQA group sizes 1, 2, 4, 8
    }
}

extern "C" int mm355_attn_decode_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                    int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                    int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                                    int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, void* stream) {
    return attn_decode_f8_impl(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt,
                               kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, 0, stream);
}
extern "C" int mm355_attn_decode_f8_variant(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                            int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                            int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o,
                                            int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant,
                                            void* stream) {
    return attn_decode_f8_impl(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt,
                               kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, variant, stream);
}

// Decode-step attention (gfx950): mm355_attn_decode(_variant) over a bf16 KV cache and mm355_attn_decode_f8(_variant) over an e4m3 one (the
// cache format of decode_kv8.hip: d bytes and ONE power-of-two fp32 scale per cached head-row).  One query row per (sample, head) against
// [kv_len] cached keys: one workgroup per 1024 cached rows (a cache bound of <= 1024 rows: per query head, no merge), partial (max, sum, o)
// per group merged by the group that arrives last.
//   * attn_decode_kernel<G, F8>: both formats from one source.  The e4m3 form differs in the width of a raw K / V load (8 bytes per lane
//     instead of 16), its unpacking, and the two scales of a key, which the thread that owns key t in the softmax phase reads and applies
//     there, once per key and never per element: the score it picks up from LDS times k_scale, the probability it puts back times v_scale.
//     x / scale is an exponent shift and fp32(byte) * scale is a bf16 value, so every fp32 value of the bf16 form on the dequantised cache is
//     reproduced exactly: the two forms are held to each other bit for bit (tests/test_kv8_gpu.py).
//   * attn_decode_split_kernel<G> (bf16, variant 1): the round-4 form, one workgroup of 256 threads per 256 keys -- the tests' second,
//     independently laid-out implementation and the baseline of tools/bench_attn_decode.py.
#include "mm355_common.h"
#include <type_traits>

namespace {

constexpr int NT = 256;
constexpr int CH = 256;                                      // keys per chunk (one per thread of a split workgroup / of a sub-block)

MM_DEV void unpack_row(const u32x4& v, float* f) { unpack8(v, f); }             // 8 bf16
MM_DEV void unpack_row(const u32x2& v, float* f) {                              // 8 e4m3
    const mm_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.x, true);
    const mm_f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, false), e = __builtin_amdgcn_cvt_pk_f32_fp8((int)v.y, true);
    f[0] = a.x; f[1] = a.y; f[2] = b.x; f[3] = b.y; f[4] = c.x; f[5] = c.y; f[6] = e.x; f[7] = e.y;
}

// The workgroup that arrives last at `counter` merges the n partial records [m, l, o[d]] of each of its G query heads (w0: the first record of
// the first head, a head's records n * (d + 2) floats apart) into the G * d outputs at o0 (round 4: no second launch).  Device-scope
// fences on both sides of the counter: the other workgroups ran on other XCDs (their records sit in other L2s until written back).  Called
// by all NTH threads of every workgroup of the (sample, KV head).
template <int G, int NTH>
MM_DEV void merge_by_last_arriver(int* counter, int n, const float* w0, int d, uint16_t* o0) {
    __shared__ int last_s;
    const int tid = threadIdx.x, rec = d + 2;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const int prev = atomicAdd(counter, 1);
        last_s = prev == n - 1;
        if (last_s) *counter = 0;                            // ready for the next launch (graph replay)
    }
    __syncthreads();
    if (!last_s) return;
    __threadfence();
    for (int i = tid; i < G * d; i += NTH) {                 // i = g * d + c
        const int g = i / d, c = i % d;
        const float* w = w0 + (int64_t)g * n * rec;
        float Mx = -INFINITY;
        for (int u = 0; u < n; ++u) Mx = fmaxf(Mx, __builtin_nontemporal_load(w + (int64_t)u * rec));
        float l = 0.f, acc1 = 0.f;
        for (int u = 0; u < n; ++u) {
            const float mm = __builtin_nontemporal_load(w + (int64_t)u * rec);
            if (mm == -INFINITY) continue;
            const float f = __expf(mm - Mx);
            l += f * __builtin_nontemporal_load(w + (int64_t)u * rec + 1);
            acc1 += f * __builtin_nontemporal_load(w + (int64_t)u * rec + 2 + c);
        }
        o0[i] = f2bf(l > 0.f ? acc1 / l : 0.f);
    }
}

// partial record per (b, q head, split): [m, l, o[d]] floats
template <int G>
__global__ __launch_bounds__(NT) void attn_decode_split_kernel(const uint16_t* __restrict__ q, int64_t ld_q, const uint16_t* __restrict__ kc,
                                                               const uint16_t* __restrict__ vc, int64_t ld_kv, int64_t bs_kv,
                                                               const int32_t* __restrict__ kv_lens, float* __restrict__ ws, int nsplit,
                                                               int Hq, int Hkv, int d, float scale, uint16_t* __restrict__ o, int64_t ld_o,
                                                               int* __restrict__ counters) {
    __shared__ float sq[G][128];                             // query rows (fp32, pre-scaled)
    __shared__ float sp[G][CH];                              // probabilities of this chunk
    __shared__ float red[G][NT / 64];
    __shared__ float so[NT / 64][G][128];                    // per-wave partial outputs
    const int s = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kv_len = kv_lens[b];
    const int rec = d + 2;
    float* wrec = ws + (((int64_t)b * Hq + hk * G) * nsplit + s) * rec;      // record of q head hk*G + g: + g * nsplit * rec
    const int k0 = s * CH;
    if (k0 >= kv_len) {                                      // chunk beyond the cache: empty partial
        if (tid < G) { float* w = wrec + (int64_t)tid * nsplit * rec; w[0] = -INFINITY; w[1] = 0.f; }
    } else {
    for (int i = tid; i < G * d; i += NT) {
        const int g = i / d, c = i % d;
        sq[g][c] = bf2f(q[(int64_t)b * ld_q + (int64_t)(hk * G + g) * d + c]) * scale;
    }
    __syncthreads();
    // ---- scores: lane = (key of a group of four, 16-B chunk of d); a wave walks its 64 keys four at a time, every K row is one
    //      coalesced 256-B read, the query chunks sit in registers, the 16 chunk partials are folded with DPP row shifts
    {
        const int dc = lane & 15, kq = lane >> 4;
        float qreg[G][8];
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) qreg[g][e] = (dc * 8 < d) ? sq[g][dc * 8 + e] : 0.f;
        // all sixteen K rows of this lane are requested before the first one is used (independent 16-B loads in flight)
        u32x4 kraw[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = k0 + wave * 64 + i * 4 + kq;
            kraw[i] = (kk < kv_len && dc * 8 < d) ? *(const u32x4*)(kc + (int64_t)b * bs_kv + (int64_t)kk * ld_kv + (int64_t)hk * d + dc * 8)
                                                  : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kl = wave * 64 + i * 4 + kq;               // key inside the chunk
            const int kk = k0 + kl;
            float kf[8];
            unpack8(kraw[i], kf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float v = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) v = fmaf(kf[e], qreg[g][e], v);
                // sum over the 16 lanes of a row: lane 15 ends up with the total
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
                if (dc == 15) sp[g][kl] = (kk < kv_len) ? v : -INFINITY;
            }
        }
    }
    __syncthreads();
    const int key = k0 + tid;
    float sc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) sc[g] = sp[g][tid];
    __syncthreads();                                         // sp is rewritten with the probabilities below
    float mx[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float w = wave_max(sc[g]);
        if (lane == 0) red[g][wave] = w;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) mx[g] = fmaxf(fmaxf(red[g][0], red[g][1]), fmaxf(red[g][2], red[g][3]));
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float p = (key < kv_len) ? __expf(sc[g] - mx[g]) : 0.f;
        sp[g][tid] = p;
        const float w = wave_sum(p);
        if (lane == 0) red[g][wave] = w;
    }
    __syncthreads();
    // ---- o = sum_key p[key] V[key]: thread = (16-B chunk of d, key group)
    const int dc = tid & 15, kg = tid >> 4;                  // 16 chunks x 16 key groups
    float acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
    {
        const int kend = min(CH, kv_len - k0);
        u32x4 vraw[16];                                      // sixteen independent 16-B loads in flight
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = kg + i * 16;
            vraw[i] = (kk < kend && dc * 8 < d) ? *(const u32x4*)(vc + (int64_t)b * bs_kv + (int64_t)(k0 + kk) * ld_kv + (int64_t)hk * d + dc * 8)
                                                : u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int kk = kg + i * 16;
            float vf[8];
            unpack8(vraw[i], vf);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float p = (kk < kend) ? sp[g][kk] : 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(p, vf[e], acc[g][e]);
            }
        }
    }
    // the four key groups of a wave are lanes l, l^16, l^32, l^48: fold them, one row of partials per wave
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = acc[g][e];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            if (lane < 16 && dc * 8 < d) so[wave][g][dc * 8 + e] = v;
        }
    __syncthreads();
    for (int i = tid; i < G * d; i += NT) {
        const int g = i / d, c = i % d;
        wrec[(int64_t)g * nsplit * rec + 2 + c] = (so[0][g][c] + so[1][g][c]) + (so[2][g][c] + so[3][g][c]);
    }
    if (tid < G) {
        float* w = wrec + (int64_t)tid * nsplit * rec;
        w[0] = mx[tid];
        w[1] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
    }
    }
    // ---- the chunk that arrives last merges the partials of its G query heads
    if (counters == nullptr) return;
    merge_by_last_arriver<G, NT>(&counters[b * Hkv + hk], nsplit, ws + (((int64_t)b * Hq + hk * G) * nsplit) * rec, d,
                                 o + (int64_t)b * ld_o + (int64_t)(hk * G) * d);
}

struct Args {
    const uint16_t* q; int64_t ld_q;
    const unsigned char* kc; const unsigned char* vc; int64_t ld_kv, bs_kv;     // BYTES per cached row / per sequence
    const float* ks; const float* vs; int64_t ld_sc, bs_sc;                     // e4m3 form: scales [B][rows][Hkv] (ignored over bf16)
    const int32_t* kv_lens; float* ws; int* counters;
    int B, Hq, d; float scale; uint16_t* o; int64_t ld_o;
};

// One workgroup of 1024 threads per (sample, head group, 1024-key group): four sub-blocks of 256 threads take one 256-key chunk each (the
// arithmetic of attn_decode_split_kernel), their partials meet in LDS, and while the cache holds <= 1024 rows the lone active workgroup
// writes the output row itself -- no workspace round trip, no device-scope fence, no counter (round 4: 23 -> ~10 us per layer at a
// 600-row cache).  Longer caches: one record per 1024-key group, merged by the group that arrives last.
// G = query heads per workgroup; Hgrp = Hq / G workgroups per sample and key group, each reading cache head (its index) / kvdiv.
template <int G, bool F8>
__global__ __launch_bounds__(1024) void attn_decode_kernel(Args a, int ngroup, int Hgrp, int kvdiv) {
    using Raw = std::conditional_t<F8, u32x2, u32x4>;                           // a lane's 8 columns of one cached row: one load
    constexpr int EB = F8 ? 1 : 2;                                              // bytes per cached element
    constexpr int SB = 4;
    constexpr int NB = G >= 8 ? 2 : (G >= 4 ? 4 : 8);                       // K / V rows per lane in flight (128 registers per thread at 16 waves per CU)
    constexpr int NBK = G == 1 ? 16 : NB;                                       // one query head: all sixteen K rows of a lane at once,
    constexpr int VPRE = G == 1 ? 16 : 0;                                       //   and its V rows issued before the softmax barriers (G = 2 spills with either)
    extern __shared__ __attribute__((aligned(16))) float lds_f[];
    float (*sp)[G][CH] = (float (*)[G][CH])(lds_f);                             // [SB][G][CH] scores, then probabilities (e4m3: * v_scale)
    float (*redm)[G][4] = (float (*)[G][4])(lds_f + SB * G * CH);               // [SB][G][4] per-wave maxima
    float (*reds)[G][4] = (float (*)[G][4])(lds_f + SB * G * CH + SB * G * 4);
    float (*so)[G][128] = (float (*)[G][128])(lds_f + SB * G * CH + 2 * SB * G * 4);   // [SB * 4 waves][G][128]
    const int grp = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, sb = tid >> 8, t = tid & 255, lane = tid & 63, wave = t >> 6;
    const int Hq = a.Hq, d = a.d;
    const int kv_len = a.kv_lens[b];
    const int ngr_live = (kv_len + SB * CH - 1) / (SB * CH);                    // groups that hold keys
    const int rec = d + 2;
    float* wrec = a.ws + (((int64_t)b * Hq + hk * G) * ngroup + grp) * rec;
    uint16_t* const orow = a.o + (int64_t)b * a.ld_o + (int64_t)(hk * G) * d;   // the G * d outputs of this workgroup's heads
    const int k0 = (grp * SB + sb) * CH;
    const bool active = k0 < kv_len;                                            // this sub-block's chunk holds keys
    // Round 6: where the time of this kernel goes.  At one sequence and a 512-row cache it moved 2 MB in 10.5 us, and the obvious reading -- a
    // chain of trips to HBM: q through LDS, two batches of K rows, three barriers of softmax, two batches of V rows -- was WRONG: with every
    // load of a thread issued up front (q straight into registers, sixteen K rows, the V rows before the softmax barriers) it took 11-14 us.
    // The workgroup is bound by INSTRUCTION ISSUE: sixteen waves on one CU = four per SIMD, each running the whole stream, and
    //   * the sub-blocks whose 256-key chunk lies beyond the cache ran it too, every lane masked off (half the waves at 512 rows): they now
    //     skip the score, softmax and PV phases (wave-uniform branches; only the barriers are shared) -- their partials were never read;
    //   * a load under a LANE predicate is a branch, and hipcc sank the whole address computation, an integer division by kvdiv included,
    //     into each of the 32 branches (~50 instructions per load): rows are now loaded unconditionally from clamped addresses (a row beyond
    //     the cache reads the last cached row, a chunk of d beyond the head reads chunk 0 -- finite values that meet a score of -inf, a
    //     probability of 0 or a store nobody makes) from two base pointers computed once;
    //   * q goes straight into the lanes' registers (no LDS copy, one barrier less).
    // Same products and the same order of additions per output as before: bit-identical results.
    const int dc8_t = ((t & 15) * 8 < d) ? (t & 15) * 8 : 0;                   // (lane & 15 == t & 15: both phases address the same chunk)
    const int hkv = hk / kvdiv;
    const unsigned char* const kbase = a.kc + (int64_t)b * a.bs_kv + ((int64_t)hkv * d + dc8_t) * EB;
    const unsigned char* const vbase = a.vc + (int64_t)b * a.bs_kv + ((int64_t)hkv * d + dc8_t) * EB;
    const int64_t ld_kv = a.ld_kv;
    if (grp * SB * CH < kv_len) {
        float ksk = 1.f, vsk = 1.f;                          // e4m3: the scales of key k0 + t (clamped as the rows are)
        if constexpr (F8) {
            if (active) {
                const int64_t so_ = (int64_t)b * a.bs_sc + (int64_t)min(k0 + t, kv_len - 1) * a.ld_sc + hkv;
                ksk = a.ks[so_];
                vsk = a.vs[so_];
            }
        }
        // ---- scores (batches of NB K rows per lane: 128 registers per thread at 16 waves per CU)
        if (active) {
            const int dc = lane & 15, kq = lane >> 4;
            float qreg[G][8];
            {
                // one 16-B load where q allows it, else eight 2-byte ones (q carries no alignment contract)
                const bool qvec = ((((uintptr_t)a.q) | ((uintptr_t)a.ld_q * 2u)) & 15u) == 0;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const uint16_t* qp = a.q + (int64_t)b * a.ld_q + (int64_t)(hk * G + g) * d + dc8_t;
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
                    for (int e = 0; e < 8; ++e) qreg[g][e] = (dc * 8 < d) ? qf[e] * a.scale : 0.f;
                }
            }
#pragma unroll 1
            for (int h = 0; h < 16 / NBK; ++h) {
                Raw kraw[NBK];
#pragma unroll
                for (int i = 0; i < NBK; ++i) {
                    const int kk = k0 + wave * 64 + (h * NBK + i) * 4 + kq;
                    kraw[i] = *(const Raw*)(kbase + (int64_t)min(kk, kv_len - 1) * ld_kv);
                }
#pragma unroll
                for (int i = 0; i < NBK; ++i) {
                    const int kl = wave * 64 + (h * NBK + i) * 4 + kq;
                    const int kk = k0 + kl;
                    float kf[8];
                    unpack_row(kraw[i], kf);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        float v = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v = fmaf(kf[e], qreg[g][e], v);
                        // sum over the 16 lanes of a row: lane 15 ends up with the total
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, true));
                        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, true));
                        if (dc == 15) sp[sb][g][kl] = (kk < kv_len) ? v : -INFINITY;
                    }
                }
            }
        }
        Raw vpre[VPRE ? VPRE : 1];
        if constexpr (VPRE > 0) {                            // the first V rows of the PV phase (its thread mapping), in flight across the softmax barriers
            if (active) {
#pragma unroll
                for (int i = 0; i < VPRE; ++i) vpre[i] = *(const Raw*)(vbase + (int64_t)min(k0 + (t >> 4) + i * 16, kv_len - 1) * ld_kv);
            }
        }
        __syncthreads();
        const int key = k0 + t;
        float sc[G];
        if (active) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sc[g] = F8 ? sp[sb][g][t] * ksk : sp[sb][g][t];                 // k_scale[key]: once per key and head (-inf stays -inf)
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
                sp[sb][g][t] = F8 ? p * vsk : p;              // (own slot: read above by this thread only.)  v_scale[key] rides on the probability; l sums the bare p
                const float w = wave_sum(p);
                if (lane == 0) reds[sb][g][wave] = w;
            }
        }
        __syncthreads();
        // ---- o = sum_key p[key] V[key]: thread = (16-B chunk of d, key group of 16), batches of NB V rows
        if (active) {
            const int dc = t & 15, kg = t >> 4;
            float acc[G][8];
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
            const int kend = min(CH, kv_len - k0);
            auto pv = [&](const Raw& vr, int kk) {
                float vf[8];
                unpack_row(vr, vf);
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
                Raw vraw[NBV];
#pragma unroll
                for (int i = 0; i < NBV; ++i) vraw[i] = *(const Raw*)(vbase + (int64_t)min(k0 + kg + (r0 + i) * 16, kv_len - 1) * ld_kv);
#pragma unroll
                for (int i = 0; i < NBV; ++i) pv(vraw[i], kg + (r0 + i) * 16);
            }
            // the four key groups of a wave are lanes l, l^16, l^32, l^48: fold them, one row of partials per wave
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
        // ---- the four chunks of this group -> one (m, l, o[d]) per query head, in a fixed order
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
            if (ngr_live == 1) {                              // the whole cache was this group's: done
                orow[i] = f2bf(l > 0.f ? acc1 / l : 0.f);
            } else {
                float* w = wrec + (int64_t)g * ngroup * rec;
                w[2 + c] = acc1;
                if (c == 0) { w[0] = Mx; w[1] = l; }
            }
        }
    } else if (ngr_live > 1 && tid < G) {                     // group beyond the cache: empty record
        float* w = wrec + (int64_t)tid * ngroup * rec;
        w[0] = -INFINITY; w[1] = 0.f;
    }
    if (ngr_live == 0 && grp == 0) {                          // an empty cache (kv_len == 0): a zero row, as the split kernel writes it
        for (int i = tid; i < G * d; i += 1024) orow[i] = 0;
    }
    if (ngr_live <= 1) return;                                // (uniform over the grid: kv_len is per sample, read by every group of it)
    merge_by_last_arriver<G, 1024>(&a.counters[b * Hgrp + hk], ngroup, wrec - (int64_t)grp * rec, d, orow);
}

// How a call is laid over workgroups: G query heads per workgroup, Hgrp = Hq / G workgroups per sample and key group, each reading cache
// head (its index) / kvdiv, and ngroup records per query head (variant 1: 256-key chunks; else 1024-key groups).
struct Plan { int G, Hgrp, kvdiv, ngroup; };

Plan make_plan(int64_t B, int64_t Hq, int64_t Hkv, int64_t max_kv_len, int variant) {
    const int G0 = (int)(Hq / Hkv);
    // a cache bound of <= 1024 rows is ONE key group: its lone workgroup per head group finishes without records or fences, so the
    // GQA group can be spread over more workgroups -- one query head each (two from 64 workgroups on): 32 workgroups instead of 8 for
    // one LLaMA-3-8B sample, 21 -> 10.5 us per launch (profiles/r5_attn_decode_heads_per_workgroup.log); the K / V rows are read by
    // every workgroup of the group (L2 hits).  Same arithmetic per head: bit-identical outputs.  Longer bounds keep the whole group in
    // one workgroup (fewer fences when the groups merge: the split forms are 2 - 4 x SLOWER there).
    // (beyond 16 sequences every CU already holds two 1024-thread workgroups: spreading the group only multiplies the K / V loads and their
    // unpacking -- measured at 32 / 64 sequences of ~520 rows: 31.1 / 55.6 us spread against 21.2 / 39.0 with the group in one workgroup;
    // 16 sequences: 17.2 against 18.8.  Same arithmetic per head either way.)
    // variant 2 = variant 0 with the whole GQA group in one workgroup whatever the bound
    if (variant == 0 && max_kv_len <= 4 * CH && (G0 == 2 || G0 == 4 || G0 == 8) && B * Hq <= 512) {
        const int gw = (B * Hq <= 64 || G0 == 2) ? 1 : 2;
        return {gw, (int)(Hq / gw), G0 / gw, 1};
    }
    const int nsplit = (int)((max_kv_len + CH - 1) / CH);
    return {G0, (int)Hkv, 1, variant == 1 ? nsplit : (nsplit + 3) / 4};
}

template <int G, bool F8>
int launch(const Args& a, const Plan& p, hipStream_t s) {
    constexpr int LDS = (4 * G * CH + 2 * 4 * G * 4 + 16 * G * 128) * 4;
    static std::atomic<uint64_t> lds_ok{0};
    if (LDS > 65536 && mm_ensure_dynamic_lds((const void*)attn_decode_kernel<G, F8>, LDS, lds_ok) != MM355_OK) return MM355_ELAUNCH;
    hipLaunchKernelGGL((attn_decode_kernel<G, F8>), dim3((unsigned)p.ngroup, (unsigned)p.Hgrp, (unsigned)a.B), dim3(1024), LDS, s, a, p.ngroup,
                       p.Hgrp, p.kvdiv);
    return mm_launch_status();
}

template <int G>
int launch_variant(const Args& a, const Plan& p, int eb, int variant, hipStream_t s) {
    if (variant == 1) {                                      // bf16 only: the strides back in elements
        hipLaunchKernelGGL(attn_decode_split_kernel<G>, dim3((unsigned)p.ngroup, (unsigned)p.Hgrp, (unsigned)a.B), dim3(NT), 0, s, a.q, a.ld_q,
                           (const uint16_t*)a.kc, (const uint16_t*)a.vc, a.ld_kv / 2, a.bs_kv / 2, a.kv_lens, a.ws, p.ngroup, a.Hq, p.Hgrp, a.d,
                           a.scale, a.o, a.ld_o, a.counters);
        return mm_launch_status();
    }
    return eb == 1 ? launch<G, true>(a, p, s) : launch<G, false>(a, p, s);
}

// the arrival counters (one per sample and KV head, Hkv <= Hq) sit at the START of the workspace, at an offset that does not depend on
// max_kv_len: one workspace serves calls with different cache lengths (the records behind them are scratch, rewritten by every launch)
int64_t decode_counter_floats(int64_t B, int64_t Hq) { return (B * Hq + 3) & ~(int64_t)3; }

// eb = bytes per cached element (2: bf16, 1: e4m3); the entry points have checked their arguments, the strides are in BYTES
int attn_decode_run(const mm355_bf16* q, int64_t ld_q, const void* k_cache, const void* v_cache, int64_t ld_kv, int64_t bs_kv, int eb,
                    const float* k_scale, const float* v_scale, int64_t ld_sc, int64_t bs_sc, const int32_t* kv_lens, int64_t max_kv_len,
                    mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant,
                    void* stream) {
    const Plan p = make_plan(B, Hq, Hkv, max_kv_len, variant);
    // counters: zero on first use (caller), left zero by every launch; behind them the per-chunk / per-group records
    const Args a = {q, ld_q, (const unsigned char*)k_cache, (const unsigned char*)v_cache, ld_kv, bs_kv, k_scale, v_scale, ld_sc, bs_sc, kv_lens,
                    workspace + decode_counter_floats(B, Hq), (int*)workspace, (int)B, (int)Hq, (int)d, scale, o, ld_o};
    hipStream_t s = (hipStream_t)stream;
    switch (p.G) {
        case 1: return launch_variant<1>(a, p, eb, variant, s);
        case 2: return launch_variant<2>(a, p, eb, variant, s);
        case 4: return launch_variant<4>(a, p, eb, variant, s);
        case 8: return launch_variant<8>(a, p, eb, variant, s);
        default: return MM355_EUNSUPPORTED;                  // GQA group sizes 1, 2, 4, 8
    }
}

int attn_decode_bf16(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                     int64_t batch_stride_kv, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq,
                     int64_t Hkv, int64_t d, float scale, float* workspace, int variant, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!q || !k_cache || !v_cache || !kv_lens || !o || !workspace || B <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || max_kv_len <= 0)
        return MM355_EINVAL;
    if (d <= 0 || d > 128 || (d & 7) || (ld_kv & 7) || (batch_stride_kv & 7) || !mm_aligned16(k_cache) || !mm_aligned16(v_cache)) return MM355_EINVAL;
    if (B > 65535 || Hkv > 65535) return MM355_EINVAL;
    if (variant < 0 || variant > 2) return MM355_EINVAL;
    return attn_decode_run(q, ld_q, k_cache, v_cache, ld_kv * 2, batch_stride_kv * 2, 2, nullptr, nullptr, 0, 0, kv_lens, max_kv_len, o, ld_o, B, Hq,
                           Hkv, d, scale, workspace, variant, stream);
}

bool aligned8(const void* p) { return (((uintptr_t)p) & 7u) == 0; }

int attn_decode_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                   int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale, int64_t batch_stride_scale, int fmt,
                   const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d,
                   float scale, float* workspace, int variant, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !q || !k_cache || !v_cache || !k_scale || !v_scale || !kv_lens || !o || !workspace || B <= 0 || Hq <= 0 ||
        Hkv <= 0 || (Hq % Hkv) || max_kv_len <= 0 || d <= 0)
        return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if ((ld_kv_bytes & 7) || (batch_stride_kv_bytes & 7) || !aligned8(k_cache) || !aligned8(v_cache) ||
        ((((uintptr_t)k_scale) | ((uintptr_t)v_scale)) & 3u) || ld_kv_bytes < Hkv * d || ld_scale < Hkv)
        return MM355_EINVAL;
    if (B > 65535 || Hkv > 65535) return MM355_EINVAL;
    if (variant != 0 && variant != 2) return MM355_EINVAL;   // the split kernel (variant 1) reads bf16 rows only
    return attn_decode_run(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, 1, k_scale, v_scale, ld_scale, batch_stride_scale, kv_lens,
                           max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, variant, stream);
}

}  // namespace

extern "C" int64_t mm355_attn_decode_ws_floats(int64_t B, int64_t Hq, int64_t d, int64_t max_kv_len) {
    if (B <= 0 || Hq <= 0 || d <= 0 || max_kv_len <= 0) return 0;
    return decode_counter_floats(B, Hq) + B * Hq * ((max_kv_len + CH - 1) / CH) * (d + 2);
}

extern "C" int mm355_attn_decode(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                 int64_t batch_stride_kv, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
                                 int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, void* stream) {
    return attn_decode_bf16(q, ld_q, k_cache, v_cache, ld_kv, batch_stride_kv, kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, 0, stream);
}
extern "C" int mm355_attn_decode_variant(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                         int64_t batch_stride_kv, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
                                         int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant, void* stream) {
    return attn_decode_bf16(q, ld_q, k_cache, v_cache, ld_kv, batch_stride_kv, kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, variant, stream);
}

extern "C" int mm355_attn_decode_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                    int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                    int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                                    int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, void* stream) {
    return attn_decode_f8(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt,
                          kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, 0, stream);
}
extern "C" int mm355_attn_decode_f8_variant(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                            int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                            int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t max_kv_len, mm355_bf16* o,
                                            int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int variant,
                                            void* stream) {
    return attn_decode_f8(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt,
                          kv_lens, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, variant, stream);
}

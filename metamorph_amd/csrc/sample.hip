// Sampled decoding in the device token loop: the counter-based uniforms (Philox4x32-10) and the row sampler that stands where the argmax
// stands (functional.GreedyLoopGraph).  The sampler draws from the distribution of HF's temperature -> top-k -> top-p -> multinomial
// without a sort: both filters keep {x_i >= tau}, tau is found by a 5-round select, and the pick walks the kept weights in index order.
// The host-side model is metamorph_amd.functional.sample_row_host.
#include "argrows.h"

#include <limits.h>
#include <math.h>

namespace {

// ------------------------------------------------------------------ Philox4x32-10 (Salmon et al., SC'11), plain integer arithmetic
MM_DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__global__ __launch_bounds__(256) void philox_uniform_rows_kernel(uint32_t k0, uint32_t k1, const int* __restrict__ stream_ids,
                                                                  const int* __restrict__ counters, float* __restrict__ u, int64_t R) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    uint32_t c[4] = {(uint32_t)counters[r], (uint32_t)stream_ids[r], 0u, 0u};
    philox4x32_10(c, k0, k1);
    u[r] = (float)(c[0] >> 8) * 0x1p-24f;                   // (24 bits: exact in fp32, < 1)
}

// ------------------------------------------------------------------ the sampler: one workgroup of 16 waves per row
constexpr int SMP_NT = 1024, SMP_NW = SMP_NT / 64;

// order-preserving key of a float that is no NaN: a < b  <=>  okey(a) < okey(b); -0 and +0 share a key
MM_DEV uint32_t okey(float x) {
    const uint32_t b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
MM_DEV float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

MM_DEV float weight(float x, float m, float inv_t) { return __expf((x - m) * inv_t); }     // (x = -inf: 0)

// round 0 of the select: 256 linear bins over [lowest finite value, m], a larger digit for a larger x.  Monotone in x (fp32 subtraction,
// multiplication by a constant >= 0 and the clamp all are), which is all the select needs; logits spread over the bins, where the top
// byte of the key would put most of a row into two or three of them (and their LDS atomics onto one address).
MM_DEV int digit0(float x, float m, float scale) {
    if (x == -INFINITY) return 0;
    const float t = (m - x) * scale;
    return 255 - (int)(t < 255.f ? t : 255.f);             // (a NaN from inf * 0 lands in the lowest bin with the other far values)
}

MM_DEV uint64_t shfl64(uint64_t v, int lane) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), lane, 64) << 32) | (uint32_t)__shfl((int)v, lane, 64);
}
MM_DEV uint64_t shfl_down64(uint64_t v, int o) {
    return ((uint64_t)(uint32_t)__shfl_down((int)(v >> 32), o, 64) << 32) | (uint32_t)__shfl_down((int)v, o, 64);
}

// f(value, column) over the columns tid, tid + 1024, ... of a row in that order (argrows.h)
template <class Fn>
MM_DEV void for_cols(const float* __restrict__ row, int C, Fn f) { row_for_cols<SMP_NT>(row, C, f); }

// Wave 0 over a 256-bin histogram: the highest bin b whose bins b .. 255 together reach `need`, and what is left of `need` inside that bin.
// frac > 0 (round 0 of the mass select): need = frac * (sum of all bins).  Integers throughout, so the order of the adds cannot matter.
template <typename T>
MM_DEV void find_bin(const T* h, uint64_t need, double frac, int* s_bin, unsigned long long* s_need) {
    const int l = threadIdx.x;
    uint64_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = h[4 * l + j];
    const uint64_t s = b[0] + b[1] + b[2] + b[3];
    uint64_t suf = s;                                        // -> the sum over the bins of lanes l .. 63
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = shfl_down64(suf, o);
        if (l + o < 64) suf += t;
    }
    const uint64_t total = shfl64(suf, 0);
    if (frac > 0.0) {
        need = (uint64_t)(frac * (double)total);
        need = need < 1 ? 1 : (need > total ? total : need);
    }
    const unsigned long long mask = __ballot(suf >= need);
    const int sel = mask ? 63 - __clzll((long long)mask) : 0;
    if (l == sel) {
        uint64_t acc = suf - s;
        int bin = 4 * l;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            if (acc + b[j] >= need) { bin = 4 * l + j; break; }
            acc += b[j];
        }
        *s_bin = bin;
        *s_need = need > acc ? need - acc : 1;
    }
}

constexpr int SMP_LIST = 8192;                             // keys of round 0's bin kept in LDS for rounds 1 .. 4

// The key of the smallest row value v (among keys >= key_lo) for which the values above it hold less than `need`: counts (MASS = false,
// need = top_k: v is the top_k-th largest value) or fixed-point weights (MASS = true, need = top_p * their sum).  Round 0 takes digit0,
// rounds 1 .. 4 the four bytes of the key of what fell into round 0's bin: from a list in LDS where the bin holds up to SMP_LIST values
// (about a hundredth of a row of logits; the list's order is arbitrary, the integer sums do not see it), else from the row again.
// Integer LDS atomics only.
template <bool MASS>
MM_DEV uint32_t select_key(const float* __restrict__ row, int C, float m, float scale, float inv_t, float wscale, uint32_t key_lo, uint64_t need,
                           double frac, uint32_t* h_cnt, unsigned long long* h_mass, uint32_t* s_keys, int* s_n, int* s_bin,
                           unsigned long long* s_need) {
    auto add = [&](int d, float xv) {
        if (MASS) atomicAdd(&h_mass[d], (unsigned long long)(weight(xv, m, inv_t) * wscale));
        else atomicAdd(&h_cnt[d], 1u);
    };
    auto clear = [&]() {
        if (threadIdx.x < 256) {
            if (MASS) h_mass[threadIdx.x] = 0; else h_cnt[threadIdx.x] = 0;
        }
        __syncthreads();
    };
    auto find = [&](double fr) {
        __syncthreads();
        if (threadIdx.x < 64) {
            if (MASS) find_bin(h_mass, need, fr, s_bin, s_need);
            else find_bin(h_cnt, need, 0.0, s_bin, s_need);
        }
        __syncthreads();
        need = *s_need;
        return *s_bin;
    };
    if (threadIdx.x == 0) *s_n = 0;
    clear();
    for_cols(row, C, [&](float xv, int) {
        if (okey(xv) >= key_lo) add(digit0(xv, m, scale), xv);
    });
    const int b0 = find(frac);
    for_cols(row, C, [&](float xv, int) {
        const uint32_t k = okey(xv);
        if (k >= key_lo && digit0(xv, m, scale) == b0) {
            const int slot = atomicAdd(s_n, 1);
            if (slot < SMP_LIST) s_keys[slot] = k;
        }
    });
    __syncthreads();
    const int n = *s_n;
    uint32_t prefix = 0;
    for (int r = 1; r < 5; ++r) {
        const int sh = 32 - 8 * r;
        auto round = [&](uint32_t k, float xv) {
            if (r > 1 && (k >> (sh + 8)) != (prefix >> (sh + 8))) return;
            add((k >> sh) & 255, xv);
        };
        clear();
        if (n <= SMP_LIST) {
            for (int i = threadIdx.x; i < n; i += SMP_NT) round(s_keys[i], okey_inv(s_keys[i]));
        } else {
            for_cols(row, C, [&](float xv, int) {
                const uint32_t k = okey(xv);
                if (k >= key_lo && digit0(xv, m, scale) == b0) round(k, xv);
            });
        }
        prefix |= (uint32_t)find(0.0) << sh;
    }
    return prefix;
}

MM_DEV float wave_incl_scan(float v) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (l >= o) v += t;
    }
    return v;
}

constexpr int SMP_NCH = 16;                                // chunks per wave span: the prefix is kept per chunk, so the pick walks one chunk

__global__ __launch_bounds__(SMP_NT) void sample_rows_kernel(const float* __restrict__ x, int C, float inv_t, int top_k, float top_p, float wscale,
                                                             const float* __restrict__ u, int* __restrict__ out, float* __restrict__ stats) {
    __shared__ float s_v[SMP_NW], s_mn[SMP_NW], s_fmn[SMP_NW], s_z[SMP_NW], s_ch[SMP_NW][SMP_NCH];
    __shared__ int s_i[SMP_NW], s_last[SMP_NW];
    __shared__ uint32_t h_cnt[256], s_keys[SMP_LIST];
    __shared__ unsigned long long h_mass[256];
    __shared__ int s_bin, s_n;
    __shared__ unsigned long long s_need;
    const int r = blockIdx.x, w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const float* row = x + (int64_t)r * C;

    // 1. the maximum with torch.argmax's index, the minimum, the lowest value above -inf: every thread ends with all four
    float v = -INFINITY, mn = INFINITY, fmn = INFINITY;
    int i = INT_MAX;
    for_cols(row, C, [&](float cv, int c) {
        if (arg_beats(cv, c, v, i)) { v = cv; i = c; }
        mn = fminf(mn, cv);
        if (cv > -INFINITY) fmn = fminf(fmn, cv);
    });
    arg_wave(v, i);
    mn = -wave_max(-mn);
    fmn = -wave_max(-fmn);
    if (l == 0) { s_v[w] = v; s_i[w] = i; s_mn[w] = mn; s_fmn[w] = fmn; }
    __syncthreads();
    v = s_v[0]; i = s_i[0]; mn = s_mn[0]; fmn = s_fmn[0];
#pragma unroll
    for (int k = 1; k < SMP_NW; ++k) {
        if (arg_beats(s_v[k], s_i[k], v, i)) { v = s_v[k]; i = s_i[k]; }
        mn = fminf(mn, s_mn[k]);
        fmn = fminf(fmn, s_fmn[k]);
    }
    const float m = v;
    if (!(fabsf(m) < INFINITY)) {                            // NaN or +inf (or a row of -inf): the argmax, no draw
        if (threadIdx.x == 0) {
            out[r] = i;
            if (stats) { stats[2 * r] = m; stats[2 * r + 1] = 0.f; }
        }
        return;
    }

    // 2. tau: the kept set is {x >= tau} = {okey(x) >= key_tau}
    const bool use_k = top_k > 0 && top_k < C, use_p = top_p < 1.f;
    uint32_t key_tau = okey(mn);
    if ((use_k || use_p) && mn < m) {
        const float span = m - fmn, sc = 256.f / span;
        const float scale = (span > 0.f && sc < INFINITY) ? sc : 0.f;
        if (use_k)
            key_tau = select_key<false>(row, C, m, scale, inv_t, wscale, 0u, (uint64_t)top_k, 0.0, h_cnt, h_mass, s_keys, &s_n, &s_bin, &s_need);
        if (use_p)
            key_tau = select_key<true>(row, C, m, scale, inv_t, wscale, key_tau, 0, (double)top_p, h_cnt, h_mass, s_keys, &s_n, &s_bin, &s_need);
    }
    auto kept_weight = [&](float cv) { return okey(cv) >= key_tau ? weight(cv, m, inv_t) : -1.f; };      // (-1: not kept)

    // 3. Z as a tree: wave w owns the columns [w * span_w, (w + 1) * span_w) in SMP_NCH chunks; per chunk a lane adds every 64th column
    //    (C / 16384 terms), the wave's butterfly makes the chunk sum; then a wave's chunk sums and the 16 wave sums in index order
    constexpr int CH_ALIGN = 64 * SMP_NCH;
    const int span_w = ((C + SMP_NW - 1) / SMP_NW + CH_ALIGN - 1) / CH_ALIGN * CH_ALIGN, chunk = span_w / SMP_NCH;
    const int64_t w_lo = (int64_t)w * span_w;
    float wz = 0.f;
    int last = -1;
    for (int j = 0; j < SMP_NCH; ++j) {
        const int64_t lo = w_lo + (int64_t)j * chunk, hi = lo + chunk < C ? lo + chunk : C;
        float acc = 0.f;
        int64_t c = lo + l;
        for (; c + 7 * 64 < hi; c += 8 * 64) {
            float cv[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) cv[t] = row[c + 64 * t];
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const float wv = kept_weight(cv[t]);
                if (wv >= 0.f) { acc += wv; last = (int)(c + 64 * t); }
            }
        }
        for (; c < hi; c += 64) {
            const float wv = kept_weight(row[c]);
            if (wv >= 0.f) { acc += wv; last = (int)c; }
        }
        acc = wave_sum(acc);
        if (l == 0) s_ch[w][j] = acc;
        wz += acc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
    if (l == 0) { s_z[w] = wz; s_last[w] = last; }
    __syncthreads();
    float Z = 0.f;
    last = -1;
#pragma unroll
    for (int k = 0; k < SMP_NW; ++k) { Z += s_z[k]; last = max(last, s_last[k]); }
    if (threadIdx.x == 0 && stats) { stats[2 * r] = okey_inv(key_tau); stats[2 * r + 1] = Z; }

    // 4. the pick: the first kept column whose inclusive prefix exceeds u * Z.  The wave in whose span the prefix of the wave sums crosses
    //    finds the chunk where its chunk sums cross and walks on from that chunk's first column, 64 columns per scan, 8 scans per trip.
    const float target = u[r] * Z;
    float base = 0.f;
    int w_pick = -1;
#pragma unroll
    for (int k = 0; k < SMP_NW; ++k) {
        if (w_pick < 0) {
            if (base + s_z[k] > target) w_pick = k; else base += s_z[k];
        }
    }
    if (w_pick < 0) {
        if (threadIdx.x == 0) out[r] = last;                 // (rounding left no column: the last kept one)
        return;
    }
    if (w != w_pick) return;
    int j_pick = 0;
    for (; j_pick < SMP_NCH - 1 && !(base + s_ch[w][j_pick] > target); ++j_pick) base += s_ch[w][j_pick];
    for (int64_t c0 = w_lo + (int64_t)j_pick * chunk; c0 < C; c0 += 8 * 64) {
        float wv[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t c = c0 + 64 * t + l;
            wv[t] = c < C ? fmaxf(kept_weight(row[c]), 0.f) : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float incl = wave_incl_scan(wv[t]);
            const unsigned long long hit = __ballot(wv[t] > 0.f && base + incl > target);
            if (hit) {
                if (l == 0) out[r] = (int)(c0 + 64 * t) + (__ffsll((long long)hit) - 1);
                return;
            }
            base += __shfl(incl, 63, 64);
        }
    }
    if (l == 0) out[r] = last;
}

}  // namespace

extern "C" int mm355_philox_uniform_rows(uint64_t seed, const int32_t* stream_ids, const int32_t* counters, float* u, int64_t R, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!stream_ids || !counters || !u || R < 1 || R > INT_MAX) return MM355_EINVAL;
    hipLaunchKernelGGL(philox_uniform_rows_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), stream_ids, counters, u, R);
    return mm_launch_status();
}

extern "C" int64_t mm355_sample_rows_ws_bytes(int64_t R, int64_t C) {
    (void)R; (void)C;
    return 0;                                                // one workgroup per row keeps its histograms in LDS
}

extern "C" int mm355_sample_rows_f32(const float* x, int64_t R, int64_t C, float inv_temperature, int top_k, float top_p, const float* u,
                                     int32_t* out, float* stats, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!x || !u || !out || R < 1 || C < 1 || C > INT_MAX - 4096 || R > 65535 || (((uintptr_t)workspace) & 3)
        || workspace_bytes < mm355_sample_rows_ws_bytes(R, C))
        return MM355_EINVAL;
    if (!(inv_temperature > 0.f) || !(inv_temperature < INFINITY) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f)) return MM355_EINVAL;
    int bits = 40;                                           // fixed-point weights: w * 2^bits, a row's sum below 2^62
    while (C > ((int64_t)1 << (62 - bits))) --bits;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)R), dim3(SMP_NT), 0, (hipStream_t)stream, x, (int)C, inv_temperature, top_k, top_p,
                       ldexpf(1.f, bits), u, out, stats);
    return mm_launch_status();
}

// Attention of n NEW rows per sequence for B sequences whose first `shared_len` cached rows are the SAME rows, stored once (gfx950): B
// questions over one context.  Row (b, i) sits at position past[b] + i; it attends the shared rows [0, shared_len) and then rows [shared_len,
// past[b] + i] of its own block (the own rows keep their absolute row index; the append comes first).  The union of attn_extend.hip (n rows,
// per-row key limit) and attn_decode_shared.hip (one copy of the first rows): n == 1 is the latter's case, shared_len == 0 the former's.
//
// Shared part: attn_decode_shared.hip's shared part with packed row r = (b * n + i) * G + g (G = the GQA group): a workgroup (KV head, 64
// packed rows, key run) reads each shared K / V tile ONCE for 64 / G query rows of any sequence.  No per-row key limit: only the ragged last
// tile is masked at shared_len.  Own part: one workgroup per (sequence, KV head, 64 of that sequence's n * G packed rows) walks the keys
// [shared_len, past[b] + n) in 64-row tiles from shared_len with attn_extend.hip's per-row limit, its skipped waves and its clamped ragged
// tiles.  Both are one launch (the own workgroups are the tail of grid x) and every workgroup writes a partial (unnormalised fp32 O, running
// maximum in the log2 domain, sum) at the row's packed index; partial slot `nsplit` is the own part.  The second launch folds the nsplit + 1
// partials of a row.  The key split depends on (B, n, Hq, Hkv, shared_len) alone.  No arrival counters, no floating-point atomics.
// The e4m3 form differs in the tile mover alone (attn_tile.h), so it equals the bf16 form on the dequantised cache bit for bit.
// Never read: rows [0, shared_len) of a sequence's own block, shared rows >= shared_len, own rows >= min(past[b] + n, max_kv_len).
#include "attn_tile.h"

namespace {
using namespace attn_tile;

struct XSArgs {
    const uint16_t* q; int64_t ld_q;
    const unsigned char* ksh; const unsigned char* vsh; int64_t ld_sh;          // shared rows, BYTES per row
    const float* kssh; const float* vssh; int64_t ld_scsh;                      // e4m3 form: their scales [shared_len][Hkv]
    const unsigned char* k; const unsigned char* v; int64_t ld_kv, bs_kv;       // own blocks, BYTES per row / per sequence
    const float* ks; const float* vs; int64_t ld_sc, bs_sc;                     // e4m3 form: scales [B][rows][Hkv]
    const int32_t* past; uint16_t* o; int64_t ld_o; float* ws;
    int n, Hkv, d, G, R, Rb, nqt, nqt_own, nsplit, tps, shared_len, max_kv; int64_t rpad;
    float scale;
};

// R packed rows in all (nqt tiles of the shared part), Rb per sequence (nqt_own tiles of the own part)
struct Plan { int G, R, Rb, nqt, nqt_own, nsplit, tps; int64_t rpad; };

// the key runs of the shared rows: attn_decode_shared.hip's rule on B * n query rows; 0 runs for an empty prefix
Plan make_plan(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t shared_len) {
    Plan p;
    p.G = (int)(Hq / Hkv);
    p.Rb = (int)(n * p.G);
    p.R = (int)(B * p.Rb);
    p.nqt = (p.R + 63) / 64;
    p.nqt_own = (p.Rb + 63) / 64;
    p.rpad = (int64_t)p.nqt * 64;
    p.nsplit = 0; p.tps = 1;
    if (shared_len > 0) key_runs(Hkv * p.nqt, (int)((shared_len + 63) / 64), p.nsplit, p.tps);
    return p;
}

template <int DP, bool F8>
__global__ __launch_bounds__(NT) void extend_shared_kernel(XSArgs a) {
    using G_ = Geo<DP>;
    constexpr int KS = G_::KS, NF = G_::NF;
    constexpr int NV = (G_::V64 + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * G_::T64];
    unsigned char* sK = smem;
    unsigned char* sV = smem + G_::T64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int hk = blockIdx.y;
    const int d = a.d, G = a.G;
    const int nshared = a.nqt * a.nsplit;
    const bool own = (int)blockIdx.x >= nshared;
    constexpr int EB = F8 ? 1 : 2;
    const int lr = wave * 16 + fr;                           // this lane's row of the workgroup

    // the workgroup's keys [k_lo, k_end) as 64-row tiles from k_lo, its packed rows [r0, r0 + nrow), its partial slot; per lane the last
    // visible key klim, per wave the smallest and the largest klim of its rows
    int k_lo, k_end, r0, nrow, slot, pr, klim, wave_lo, wave_hi;
    const unsigned char* kbase; const unsigned char* vbase; const float* ksb = nullptr; const float* vsb = nullptr;
    int64_t ld, ld_sc;
    if (own) {
        const int idx = (int)blockIdx.x - nshared;
        const int b = idx / a.nqt_own, q0 = (idx - b * a.nqt_own) * 64, qw0 = q0 + wave * 16;
        const int Rb = a.Rb, past = a.past[b];
        k_lo = a.shared_len;
        // last key (exclusive) any row of this workgroup sees; the host bound keeps a wrong past[] inside the cache
        k_end = min(past + min(Rb - 1, q0 + 63) / G + 1, a.max_kv);
        nrow = min(64, Rb - q0); slot = a.nsplit;
        r0 = b * Rb + q0;
        pr = r0 + min(lr, nrow - 1);
        klim = past + min(q0 + lr, Rb - 1) / G;
        wave_lo = past + min(qw0, Rb - 1) / G; wave_hi = past + min(qw0 + 15, Rb - 1) / G;
        kbase = a.k + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
        vbase = a.v + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
        if (F8) { ksb = a.ks + (int64_t)b * a.bs_sc + hk; vsb = a.vs + (int64_t)b * a.bs_sc + hk; }
        ld = a.ld_kv; ld_sc = a.ld_sc;
    } else {
        const int qt = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
        k_lo = split * a.tps * 64;
        k_end = min(a.shared_len, k_lo + a.tps * 64);
        r0 = qt * 64; nrow = min(64, a.R - r0); slot = split;
        pr = r0 + min(lr, nrow - 1);
        klim = wave_lo = wave_hi = k_end - 1;                // every row sees every shared key
        kbase = a.ksh + (int64_t)hk * d * EB;
        vbase = a.vsh + (int64_t)hk * d * EB;
        if (F8) { ksb = a.kssh + hk; vsb = a.vssh + hk; }
        ld = a.ld_sh; ld_sc = a.ld_scsh;
    }
    const int ntiles = k_end > k_lo ? (k_end - k_lo + 63) >> 6 : 0;
    const int qrow = pr / G, qg = pr - qrow * G;             // packed row -> query row b * n + i and head of the group
    const bool wave_on = wave * 16 < nrow;

    bf16x8 qf[KS];                                           // B operand: Q[row = fr][d chunk]
    {
        const uint16_t* qp = a.q + (int64_t)qrow * a.ld_q + (int64_t)(hk * G + qg) * d;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int c = kk * 32 + fq * 8;
            qf[kk] = (c < d) ? *(const bf16x8*)(qp + c) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    f32x4 ot[NF];                                            // O^T[d = j*16 + fq*4 + r][row = fr]
    float m_run = -INFINITY, l_run = 0.f;
#pragma unroll
    for (int j = 0; j < NF; ++j) ot[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float sl2 = a.scale * 1.4426950408889634f;         // scores in log2 domain: exp2(s*sl2 - m), the scale on the fp32 side

    if (ntiles > 0) {
        Stage<NV, F8> rk, rv;
        load_tile<DP, NV, F8>(rk, kbase, ksb, ld, ld_sc, k_lo, k_end, d, tid);
        load_tile<DP, NV, F8>(rv, vbase, vsb, ld, ld_sc, k_lo, k_end, d, tid);
        store_tile<DP, NV, F8>(rk, sK, tid);
        store_tile<DP, NV, F8>(rv, sV, tid);
        __syncthreads();
        for (int t = 0; t < ntiles; ++t) {
            const int kv0 = k_lo + t * 64;
            const bool more = t + 1 < ntiles;
            if (more) {
                load_tile<DP, NV, F8>(rk, kbase, ksb, ld, ld_sc, kv0 + 64, k_end, d, tid);
                load_tile<DP, NV, F8>(rv, vbase, vsb, ld, ld_sc, kv0 + 64, k_end, d, tid);
            }
            if (wave_on && kv0 <= wave_hi)                   // a wave whose rows all precede this tile has nothing to do here
                softmax_tile<DP>(sK, sV, qf, ot, m_run, l_run, kv0, kv0 + 63 > wave_lo, klim, sl2, fr, fq);
            __syncthreads();                                 // every wave is done reading this tile
            if (more) {
                store_tile<DP, NV, F8>(rk, sK, tid);
                store_tile<DP, NV, F8>(rv, sV, tid);
                __syncthreads();
            }
        }
    }

    if (lr < nrow) {                                         // partial: unnormalised O, reference maximum (log2 domain) and sum
        const int64_t row = ((int64_t)hk * (a.nsplit + 1) + slot) * a.rpad + pr;
        float* po = a.ws + row * DP;
#pragma unroll
        for (int j = 0; j < NF; ++j) *(f32x4*)(po + j * 16 + fq * 4) = ot[j];
        if (fq == 0) {
            float* ml = a.ws + (int64_t)a.Hkv * (a.nsplit + 1) * a.rpad * DP + row * 2;
            ml[0] = m_run; ml[1] = l_run;
        }
    }
}

// o[b * n + i][head][4 columns] from the nsplit + 1 partials of packed row (b * n + i) * G + g
template <int DP>
__global__ __launch_bounds__(NT) void extend_shared_merge_kernel(XSArgs a) {
    const int hk = blockIdx.y;
    const int64_t idx = (int64_t)blockIdx.x * NT + threadIdx.x;
    const int p = (int)(idx / (DP / 4)), c = (int)(idx % (DP / 4)) * 4;
    if (p >= a.R || c >= a.d) return;
    const int nslots = a.nsplit + 1;
    const int64_t row0 = (int64_t)hk * nslots * a.rpad + p;
    const float* ml = a.ws + (int64_t)a.Hkv * nslots * a.rpad * DP;
    const u32x2 w = merge_partials<DP>(a.ws, ml, row0, a.rpad, nslots, c);
    const int qrow = p / a.G, g = p - qrow * a.G;
    *(u32x2*)(a.o + (int64_t)qrow * a.ld_o + (int64_t)(hk * a.G + g) * a.d + c) = w;
}

template <int DP, bool F8>
int launch(const XSArgs& a, int64_t B, hipStream_t s) {
    const unsigned gx = (unsigned)((int64_t)a.nqt * a.nsplit + B * a.nqt_own);
    hipLaunchKernelGGL((extend_shared_kernel<DP, F8>), dim3(gx, (unsigned)a.Hkv), dim3(NT), 0, s, a);
    if (mm_launch_status() != MM355_OK) return MM355_ELAUNCH;
    const unsigned gm = (unsigned)(((int64_t)a.R * (DP / 4) + NT - 1) / NT);
    hipLaunchKernelGGL((extend_shared_merge_kernel<DP>), dim3(gm, (unsigned)a.Hkv), dim3(NT), 0, s, a);
    return mm_launch_status();
}

int pick_dp(int64_t d) { return d <= 64 ? 64 : (d <= 96 ? 96 : 128); }

int64_t ws_floats(const Plan& p, int64_t Hkv, int64_t d) { return Hkv * (p.nsplit + 1) * p.rpad * (pick_dp(d) + 2); }

// what mm355_attn_decode_shared refuses about the shape, and n
bool shape_ok(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len, int64_t max_kv_len) {
    return B > 0 && n > 0 && Hq > 0 && Hkv > 0 && !(Hq % Hkv) && d > 0 && max_kv_len > 0 && n <= max_kv_len && shared_len >= 0 &&
           shared_len <= max_kv_len && max_kv_len <= 0x7fffffc0ll && B <= 0x7ffffffll && n <= 0x7fffffc0ll &&
           B * n <= 0x7fffffc0ll / (Hq / Hkv) && Hkv <= 65535;
}

// eb = bytes per cached element (2: bf16, 1: e4m3); the row and sequence strides arrive in BYTES
int extend_shared_impl(const mm355_bf16* q, int64_t ld_q, const void* ksh, const void* vsh, int64_t ld_sh, const float* kssh, const float* vssh,
                       int64_t ld_scsh, const void* k, const void* v, int64_t ld_kv, int64_t bs_kv, int eb, const float* ks, const float* vs,
                       int64_t ld_sc, int64_t bs_sc, const int32_t* past, int64_t n, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o,
                       int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* ws, int64_t ws_fl, void* stream) {
    if (!q || !ksh || !vsh || !k || !v || !past || !o || !shape_ok(B, n, Hq, Hkv, d, shared_len, max_kv_len)) return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    const uintptr_t amask = eb == 2 ? 15u : 7u;              // one 16-byte (bf16) or 8-byte (e4m3) load per 8 columns
    if (!mm_aligned16(q) || !mm_aligned16(o) || (ld_q & 7) || (ld_o & 7) || ld_q < Hq * d || ld_o < Hq * d ||
        (((uintptr_t)k | (uintptr_t)v | (uintptr_t)ksh | (uintptr_t)vsh) & amask) || ((ld_kv | bs_kv | ld_sh) & (int64_t)amask) ||
        ld_kv < Hkv * d * eb || ld_sh < Hkv * d * eb)
        return MM355_EINVAL;
    if (eb == 1 && (((((uintptr_t)ks) | ((uintptr_t)vs) | ((uintptr_t)kssh) | ((uintptr_t)vssh)) & 3u) || ld_sc < Hkv || ld_scsh < Hkv))
        return MM355_EINVAL;
    const int64_t G = Hq / Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return MM355_EUNSUPPORTED;      // GQA group sizes 1, 2, 4, 8
    const Plan p = make_plan(B, n, Hq, Hkv, shared_len);
    if ((int64_t)p.nqt * p.nsplit + B * p.nqt_own > 0x7fffffffll) return MM355_EINVAL;
    if (!ws || (((uintptr_t)ws) & 15u) || ws_fl < ws_floats(p, Hkv, d)) return MM355_EINVAL;
    XSArgs a{q, ld_q, (const unsigned char*)ksh, (const unsigned char*)vsh, ld_sh, kssh, vssh, ld_scsh, (const unsigned char*)k,
             (const unsigned char*)v, ld_kv, bs_kv, ks, vs, ld_sc, bs_sc, past, o, ld_o, ws, (int)n, (int)Hkv, (int)d, p.G, p.R, p.Rb, p.nqt,
             p.nqt_own, p.nsplit, p.tps, (int)shared_len, (int)max_kv_len, p.rpad, scale};
    hipStream_t s = (hipStream_t)stream;
    const int dp = pick_dp(d);
    if (eb == 2) {
        switch (dp) {
            case 64: return launch<64, false>(a, B, s);
            case 96: return launch<96, false>(a, B, s);
            default: return launch<128, false>(a, B, s);
        }
    }
    switch (dp) {
        case 64: return launch<64, true>(a, B, s);
        case 96: return launch<96, true>(a, B, s);
        default: return launch<128, true>(a, B, s);
    }
}

}  // namespace

extern "C" int64_t mm355_attn_extend_shared_ws_floats(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len,
                                                      int64_t max_kv_len) {
    if (!shape_ok(B, n, Hq, Hkv, d, shared_len, max_kv_len) || d > 128) return 0;
    return ws_floats(make_plan(B, n, Hq, Hkv, shared_len), Hkv, d);
}

extern "C" int mm355_attn_extend_shared(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared,
                                        int64_t ld_shared, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                        int64_t batch_stride_kv, const int32_t* past, int64_t n, int64_t shared_len, int64_t max_kv_len,
                                        mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                                        float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    return extend_shared_impl(q, ld_q, k_shared, v_shared, ld_shared * 2, nullptr, nullptr, 0, k_cache, v_cache, ld_kv * 2, batch_stride_kv * 2, 2,
                              nullptr, nullptr, 0, 0, past, n, shared_len, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats,
                              stream);
}

extern "C" int mm355_attn_extend_shared_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared,
                                           int64_t ld_shared_bytes, const float* k_shared_scale, const float* v_shared_scale,
                                           int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                           int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                           int64_t batch_stride_scale, int fmt, const int32_t* past, int64_t n, int64_t shared_len,
                                           int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d,
                                           float scale, float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !k_scale || !v_scale || !k_shared_scale || !v_shared_scale) return MM355_EINVAL;
    return extend_shared_impl(q, ld_q, k_shared, v_shared, ld_shared_bytes, k_shared_scale, v_shared_scale, ld_shared_scale, k_cache, v_cache,
                              ld_kv_bytes, batch_stride_kv_bytes, 1, k_scale, v_scale, ld_scale, batch_stride_scale, past, n, shared_len, max_kv_len,
                              o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

// Attention of n >= 1 NEW rows per sequence for B sequences whose first `shared_len` cached rows are the SAME rows, stored once (gfx950): B
// questions over one context (mm355_attn_extend_shared), and with n == 1 the decode step of n sampled continuations or beams of one prompt
// (mm355_attn_decode_shared, which hands over kv_lens = past + 1).  Row (b, i) sits at position past[b] + i; it attends the shared rows [0,
// shared_len) and then rows [shared_len, past[b] + i] of its own block (the own rows keep their absolute row index, so the append kernels'
// position is still the cache row; the append comes first).  shared_len == 0 is attn_extend.hip's case.
//
// Shared part: attn_extend.hip's tile walk with packed row r = (b * n + i) * G + g (G = the GQA group): a workgroup (KV head, 64 packed rows,
// key run) reads each shared K / V tile ONCE for 64 / G query rows of any sequence.  No per-row key limit: only the ragged last tile is
// masked at shared_len.  Own part: one workgroup per (sequence, KV head, 64 of that sequence's n * G packed rows) walks the keys
// [shared_len, past[b] + n) in 64-row tiles from shared_len with attn_extend.hip's per-row limit, its skipped waves and its clamped ragged
// tiles; with n == 1 that is one workgroup per (sequence, KV head) whose G rows all stop at past[b].  Both are one launch (the own workgroups
// are the tail of grid x) and every workgroup writes a partial (unnormalised fp32 O, running maximum in the log2 domain, sum) at the row's
// packed index; partial slot `nsplit` is the own part.  The second launch folds the nsplit + 1 partials of a row.  The key split depends on
// (B, n, Hq, Hkv, shared_len) alone.  No arrival counters, no floating-point atomics.
// The e4m3 form differs in the tile mover alone (attn_tile.h), so it equals the bf16 form on the dequantised cache bit for bit.
// Never read: rows [0, shared_len) of a sequence's own block, shared rows >= shared_len, own rows >= min(past[b] + n, max_kv_len).
// The indexed form (the beams of a beam search, functional.BeamLoopGraph; one row per sequence): own row j of sequence b is row j of the block
// own_block[b][j - shared_len], one byte per row.  The own workgroup fetches the entries of the tile after next with the rows of the next
// tile, so the dependent load in front of a row's address has a tile's compute to arrive.  It is a kernel of its own, shared_idx_kernel, on
// the same pieces, the same grid, workspace and merge.
#include "attn_tile.h"

namespace {
using namespace attn_tile;

struct XSArgs {
    const uint16_t* q; int64_t ld_q;
    const unsigned char* ksh; const unsigned char* vsh; int64_t ld_sh;          // shared rows, BYTES per row
    const float* kssh; const float* vssh; int64_t ld_scsh;                      // e4m3 form: their scales [shared_len][Hkv]
    const unsigned char* k; const unsigned char* v; int64_t ld_kv, bs_kv;       // own blocks, BYTES per row / per sequence
    const float* ks; const float* vs; int64_t ld_sc, bs_sc;                     // e4m3 form: scales [B][rows][Hkv]
    const int32_t* lens; int len_off;                                           // past[b] = lens[b] - len_off (0: past[], 1: kv_lens[])
    uint16_t* o; int64_t ld_o; float* ws;
    const uint8_t* own_block; int64_t ld_ob;                                    // indexed form: block of own row t of sequence b at [b * ld_ob + t]
    int B, Hkv, d, G, R, Rb, nqt, nqt_own, nsplit, tps, shared_len, max_kv; int64_t rpad;
    float scale;
};

// R packed rows in all (nqt tiles of the shared part), Rb per sequence (nqt_own tiles of the own part)
struct Plan { int G, R, Rb, nqt, nqt_own, nsplit, tps; int64_t rpad; };

// the key runs of the shared rows: attn_extend.hip's rule (runs of >= 4 key tiles until there is about one workgroup per CU) on the B * n
// query rows; 0 runs for an empty prefix
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
    constexpr int KS = G_::KS, NF = G_::NF, NV = tile_nv<DP>;
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

    // the workgroup's keys [k_lo, k_end) as 64-row tiles from k_lo, its packed rows [r0, r0 + nrow), its partial slot and, for the own part,
    // klim0 = past[b] less the sequence's first query row b * n: query row b * n + i stops at key klim0 + b * n + i
    int k_lo, k_end, r0, nrow, slot, klim0 = 0;
    const unsigned char* kbase; const unsigned char* vbase; const float* ksb = nullptr; const float* vsb = nullptr;
    int64_t ld, ld_sc;
    if (own) {
        const int idx = (int)blockIdx.x - nshared;
        const int b = idx / a.nqt_own, q0 = (idx - b * a.nqt_own) * 64;
        const int Rb = a.Rb, past = a.lens[b] - a.len_off;
        k_lo = a.shared_len;
        // last key (exclusive) any row of this workgroup sees; the host bound keeps a wrong length inside the cache
        k_end = min(past + min(Rb - 1, q0 + 63) / G + 1, a.max_kv);
        nrow = min(64, Rb - q0); slot = a.nsplit;
        r0 = b * Rb + q0;
        klim0 = past - b * (Rb / G);
        kbase = a.k + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
        vbase = a.v + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
        if (F8) { ksb = a.ks + (int64_t)b * a.bs_sc + hk; vsb = a.vs + (int64_t)b * a.bs_sc + hk; }
        ld = a.ld_kv; ld_sc = a.ld_sc;
    } else {
        const int qt = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
        k_lo = split * a.tps * 64;
        k_end = min(a.shared_len, k_lo + a.tps * 64);
        r0 = qt * 64; nrow = min(64, a.R - r0); slot = split;
        kbase = a.ksh + (int64_t)hk * d * EB;
        vbase = a.vsh + (int64_t)hk * d * EB;
        if (F8) { ksb = a.kssh + hk; vsb = a.vssh + hk; }
        ld = a.ld_sh; ld_sc = a.ld_scsh;
    }
    const int ntiles = k_end > k_lo ? (k_end - k_lo + 63) >> 6 : 0;
    const int pr = r0 + min(lr, nrow - 1);                   // this lane's packed row (clamped: rows >= nrow are not stored)
    const int qrow = pr / G, qg = pr - qrow * G;             // packed row -> query row b * n + i and head of the group
    // The lane's last visible key and the smallest and the largest of its wave.  Own part: row i of the sequence stops at past[b] + i, which
    // is min(q0 + lr, Rb - 1) / G past past[b]; the packed row's division has it already, and a wave's first and last rows are its lanes 0
    // and 15, so the three divisions of the n-row kernel this came from are not repeated: the one-row decode step pays for them otherwise
    // (its launch measured 1 % slower).  Shared part: every row sees every key.
    const int klim = own ? klim0 + qrow : k_end - 1;
    const int wave_lo = __builtin_amdgcn_readlane(klim, 0), wave_hi = __builtin_amdgcn_readlane(klim, 15);
    const bool wave_on = wave * 16 < nrow;

    bf16x8 qf[KS];
    {
        const uint16_t* qp = a.q + (int64_t)qrow * a.ld_q + (int64_t)(hk * G + qg) * d;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = load_q(qp, kk, d, fq);
    }
    f32x4 ot[NF];
    float m_run, l_run;
    init_acc<DP>(ot, m_run, l_run);
    const float sl2 = a.scale * 1.4426950408889634f;         // scores in log2 domain: exp2(s*sl2 - m), the scale on the fp32 side

    auto fetch = [&](Stage<NV, F8>& rk, Stage<NV, F8>& rv, int row0, int end) {
        load_tile<DP, NV, F8>(rk, kbase, ksb, ld, ld_sc, row0, end, d, tid);
        load_tile<DP, NV, F8>(rv, vbase, vsb, ld, ld_sc, row0, end, d, tid);
    };
    walk_tiles<DP, F8>(fetch, sK, sV, qf, ot, m_run, l_run, k_lo, ntiles, k_end, wave_on, wave_lo, wave_hi, klim, sl2, tid, fr, fq);

    if (lr < nrow)
        store_partial<DP>(a.ws, (int64_t)a.Hkv * (a.nsplit + 1) * a.rpad, ((int64_t)hk * (a.nsplit + 1) + slot) * a.rpad + pr, ot, m_run, l_run, fq);
}

// The indexed form, one row per sequence (Rb = G, one own workgroup per sequence and KV head): the shared part as above, the own part with
// a uniform key limit kv_lens[b] - 1 and the table in front of every row's address.  Kept apart from extend_shared_kernel: as an IDX
// instance of that kernel the d = 96 e4m3 form needs 152 - 156 registers for this one's 128 (4 -> 3 waves per SIMD): the n-row map's
// per-lane limits and the table's look-ahead do not fit one register budget.  Same pieces, same grid, same workspace, same merge.
template <int DP, bool F8>
__global__ __launch_bounds__(NT) void shared_idx_kernel(XSArgs a) {
    using G_ = Geo<DP>;
    constexpr int KS = G_::KS, NF = G_::NF, NV = tile_nv<DP>;
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

    int k_lo, k_end, r0, nrow, slot;
    const unsigned char* kbase; const unsigned char* vbase; const float* ksb = nullptr; const float* vsb = nullptr;
    int64_t ld, ld_sc;
    if (own) {
        const int b = (int)blockIdx.x - nshared;
        k_lo = a.shared_len;
        k_end = min(a.lens[b] - a.len_off + 1, a.max_kv);    // the host bound keeps a wrong length inside the cache
        r0 = b * G; nrow = G; slot = a.nsplit;
        kbase = a.k + (int64_t)hk * d * EB;                  // (the block comes per row, from the table)
        vbase = a.v + (int64_t)hk * d * EB;
        if (F8) { ksb = a.ks + hk; vsb = a.vs + hk; }
        ld = a.ld_kv; ld_sc = a.ld_sc;
    } else {
        const int qt = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
        k_lo = split * a.tps * 64;
        k_end = min(a.shared_len, k_lo + a.tps * 64);
        r0 = qt * 64; nrow = min(64, a.R - r0); slot = split;
        kbase = a.ksh + (int64_t)hk * d * EB;
        vbase = a.vsh + (int64_t)hk * d * EB;
        if (F8) { ksb = a.kssh + hk; vsb = a.vssh + hk; }
        ld = a.ld_sh; ld_sc = a.ld_scsh;
    }
    const int ntiles = k_end > k_lo ? (k_end - k_lo + 63) >> 6 : 0;
    const int lr = wave * 16 + fr;                           // this lane's row of the workgroup
    const int pr = r0 + min(lr, nrow - 1);                   // its packed row (clamped: rows >= nrow are not stored)
    const int qb = pr / G, qg = pr - qb * G;
    const bool wave_on = wave * 16 < nrow;

    bf16x8 qf[KS];
    {
        const uint16_t* qp = a.q + (int64_t)qb * a.ld_q + (int64_t)(hk * G + qg) * d;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = load_q(qp, kk, d, fq);
    }
    f32x4 ot[NF];
    float m_run, l_run;
    init_acc<DP>(ot, m_run, l_run);
    const float sl2 = a.scale * 1.4426950408889634f;         // scores in log2 domain: exp2(s*sl2 - m), the scale on the fp32 side

    if (ntiles > 0) {                                        // (the table's state lives in this scope: outside it costs registers)
        int blk[NV];                                         // own rows: the blocks of the tile `fetch` moves next
        const uint8_t* tbl = nullptr;
        if (own) {
            tbl = a.own_block + (int64_t)((int)blockIdx.x - nshared) * a.ld_ob;
            load_blocks<DP, NV>(blk, tbl, (int)a.ld_ob, a.B, a.shared_len, k_lo, k_end, tid);
        }
        auto fetch = [&](Stage<NV, F8>& rk, Stage<NV, F8>& rv, int row0, int end) {
            if (own) {
                load_tile_idx<DP, NV, F8>(rk, kbase, ksb, ld, ld_sc, a.bs_kv, a.bs_sc, blk, row0, end, d, tid);
                load_tile_idx<DP, NV, F8>(rv, vbase, vsb, ld, ld_sc, a.bs_kv, a.bs_sc, blk, row0, end, d, tid);
                load_blocks<DP, NV>(blk, tbl, (int)a.ld_ob, a.B, a.shared_len, row0 + 64, end, tid);
                return;
            }
            load_tile<DP, NV, F8>(rk, kbase, ksb, ld, ld_sc, row0, end, d, tid);
            load_tile<DP, NV, F8>(rv, vbase, vsb, ld, ld_sc, row0, end, d, tid);
        };
        // every row of the workgroup sees all of its keys: one limit, only the ragged last tile is masked
        walk_tiles<DP, F8>(fetch, sK, sV, qf, ot, m_run, l_run, k_lo, ntiles, k_end, wave_on, k_end - 1, k_end - 1, k_end - 1, sl2, tid, fr, fq);
    }

    if (lr < nrow)
        store_partial<DP>(a.ws, (int64_t)a.Hkv * (a.nsplit + 1) * a.rpad, ((int64_t)hk * (a.nsplit + 1) + slot) * a.rpad + pr, ot, m_run, l_run, fq);
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
int launch(const XSArgs& a, hipStream_t s) {
    const dim3 grid((unsigned)((int64_t)a.nqt * a.nsplit + (int64_t)a.B * a.nqt_own), (unsigned)a.Hkv);
    if (a.own_block) hipLaunchKernelGGL((shared_idx_kernel<DP, F8>), grid, dim3(NT), 0, s, a);
    else hipLaunchKernelGGL((extend_shared_kernel<DP, F8>), grid, dim3(NT), 0, s, a);
    if (mm_launch_status() != MM355_OK) return MM355_ELAUNCH;
    const unsigned gm = (unsigned)(((int64_t)a.R * (DP / 4) + NT - 1) / NT);
    hipLaunchKernelGGL((extend_shared_merge_kernel<DP>), dim3(gm, (unsigned)a.Hkv), dim3(NT), 0, s, a);
    return mm_launch_status();
}

int64_t ws_floats(const Plan& p, int64_t Hkv, int64_t d) { return Hkv * (p.nsplit + 1) * p.rpad * (pick_dp(d) + 2); }

// what every entry point refuses about the counts
bool shape_ok(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len, int64_t max_kv_len) {
    return B > 0 && n > 0 && Hq > 0 && Hkv > 0 && !(Hq % Hkv) && d > 0 && max_kv_len > 0 && n <= max_kv_len && shared_len >= 0 &&
           shared_len <= max_kv_len && max_kv_len <= 0x7fffffc0ll && B <= 0x7ffffffll && n <= 0x7fffffc0ll &&
           B * n <= 0x7fffffc0ll / (Hq / Hkv) && Hkv <= 65535;
}

// n rows per sequence at past[b] = lens[b] - len_off; eb = bytes per cached element (2: bf16, 1: e4m3), the strides of `sh` and `own` in
// BYTES; own_block NULL: every own row in its sequence's block
int impl(const mm355_bf16* q, int64_t ld_q, const CacheRef& sh, const CacheRef& own, int eb, const int32_t* lens, int len_off,
         const uint8_t* own_block, int64_t ld_ob, int64_t n, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
         int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* ws, int64_t ws_fl, void* stream) {
    if (const int rc = refuse(lens && shape_ok(B, n, Hq, Hkv, d, shared_len, max_kv_len) &&
                                  // the table: one byte names a block, and shared_idx_kernel is a one-row kernel (no entry point
                                  // pairs a table with n > 1)
                                  !(own_block && (n != 1 || B > 255 || ld_ob < 1 || ld_ob > 0x7fffffffll)),
                              q, ld_q, o, ld_o, own, &sh, eb, Hq, Hkv, d))
        return rc;
    const Plan p = make_plan(B, n, Hq, Hkv, shared_len);
    if ((int64_t)p.nqt * p.nsplit + B * p.nqt_own > 0x7fffffffll) return MM355_EINVAL;
    if (!ws || (((uintptr_t)ws) & 15u) || ws_fl < ws_floats(p, Hkv, d)) return MM355_EINVAL;
    XSArgs a{q, ld_q, (const unsigned char*)sh.k, (const unsigned char*)sh.v, sh.ld, sh.ks, sh.vs, sh.ld_sc, (const unsigned char*)own.k,
             (const unsigned char*)own.v, own.ld, own.bs, own.ks, own.vs, own.ld_sc, own.bs_sc, lens, len_off, o, ld_o, ws, own_block, ld_ob, (int)B,
             (int)Hkv, (int)d, p.G, p.R, p.Rb, p.nqt, p.nqt_own, p.nsplit, p.tps, (int)shared_len, (int)max_kv_len, p.rpad, scale};
    return dispatch(eb, d, [&](auto dp, auto f8) { return launch<decltype(dp)::value, decltype(f8)::value>(a, (hipStream_t)stream); });
}

// the bf16 entry points: strides in elements, no scales
int impl_bf16(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared, int64_t ld_shared,
              const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv, int64_t batch_stride_kv, const int32_t* lens, int len_off,
              const uint8_t* own_block, int64_t ld_ob, int64_t n, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B,
              int64_t Hq, int64_t Hkv, int64_t d, float scale, float* ws, int64_t ws_fl, void* stream) {
    (void)hipGetLastError();
    return impl(q, ld_q, CacheRef{k_shared, v_shared, ld_shared * 2, 0, nullptr, nullptr, 0, 0},
                CacheRef{k_cache, v_cache, ld_kv * 2, batch_stride_kv * 2, nullptr, nullptr, 0, 0}, 2, lens, len_off, own_block, ld_ob, n, shared_len,
                max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, ws, ws_fl, stream);
}

// the e4m3 entry points: strides in bytes, scales for both sets of rows
int impl_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared, int64_t ld_shared_bytes,
            const float* k_shared_scale, const float* v_shared_scale, int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache,
            int64_t ld_kv_bytes, int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
            int64_t batch_stride_scale, int fmt, const int32_t* lens, int len_off, const uint8_t* own_block, int64_t ld_ob, int64_t n,
            int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
            float* ws, int64_t ws_fl, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !k_scale || !v_scale || !k_shared_scale || !v_shared_scale) return MM355_EINVAL;
    return impl(q, ld_q, CacheRef{k_shared, v_shared, ld_shared_bytes, 0, k_shared_scale, v_shared_scale, ld_shared_scale, 0},
                CacheRef{k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale}, 1, lens, len_off,
                own_block, ld_ob, n, shared_len, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, ws, ws_fl, stream);
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
    return impl_bf16(q, ld_q, k_shared, v_shared, ld_shared, k_cache, v_cache, ld_kv, batch_stride_kv, past, 0, nullptr, 0, n, shared_len, max_kv_len,
                     o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_extend_shared_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared,
                                           int64_t ld_shared_bytes, const float* k_shared_scale, const float* v_shared_scale,
                                           int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                           int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                           int64_t batch_stride_scale, int fmt, const int32_t* past, int64_t n, int64_t shared_len,
                                           int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d,
                                           float scale, float* workspace, int64_t workspace_floats, void* stream) {
    return impl_f8(q, ld_q, k_shared, v_shared, ld_shared_bytes, k_shared_scale, v_shared_scale, ld_shared_scale, k_cache, v_cache, ld_kv_bytes,
                   batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt, past, 0, nullptr, 0, n, shared_len, max_kv_len, o, ld_o,
                   B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

// The decode step's entry points: one row per sequence, handed over as kv_lens[b] = past[b] + 1; the indexed ones add the table.

extern "C" int64_t mm355_attn_decode_shared_ws_floats(int64_t B, int64_t Hq, int64_t Hkv, int64_t d, int64_t shared_len, int64_t max_kv_len) {
    // (0 for every shape the entry points refuse: without the upper limits of shape_ok a B * G beyond int would leave the plan no row tile
    // and key_runs a division by zero)
    return mm355_attn_extend_shared_ws_floats(B, 1, Hq, Hkv, d, shared_len, max_kv_len);
}

extern "C" int mm355_attn_decode_shared(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared,
                                        int64_t ld_shared, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                        int64_t batch_stride_kv, const int32_t* kv_lens, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o,
                                        int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace,
                                        int64_t workspace_floats, void* stream) {
    return impl_bf16(q, ld_q, k_shared, v_shared, ld_shared, k_cache, v_cache, ld_kv, batch_stride_kv, kv_lens, 1, nullptr, 0, 1, shared_len,
                     max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_decode_shared_idx(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_shared, const mm355_bf16* v_shared,
                                            int64_t ld_shared, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                            int64_t batch_stride_kv, const int32_t* kv_lens, const uint8_t* own_block, int64_t ld_own_block,
                                            int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq,
                                            int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream) {
    return impl_bf16(q, ld_q, k_shared, v_shared, ld_shared, k_cache, v_cache, ld_kv, batch_stride_kv, kv_lens, 1, own_block, ld_own_block, 1,
                     shared_len, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_decode_shared_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared,
                                           int64_t ld_shared_bytes, const float* k_shared_scale, const float* v_shared_scale,
                                           int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                           int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                           int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, int64_t shared_len, int64_t max_kv_len,
                                           mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                                           float* workspace, int64_t workspace_floats, void* stream) {
    return impl_f8(q, ld_q, k_shared, v_shared, ld_shared_bytes, k_shared_scale, v_shared_scale, ld_shared_scale, k_cache, v_cache, ld_kv_bytes,
                   batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt, kv_lens, 1, nullptr, 0, 1, shared_len, max_kv_len, o,
                   ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_decode_shared_idx_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_shared, const uint8_t* v_shared,
                                               int64_t ld_shared_bytes, const float* k_shared_scale, const float* v_shared_scale,
                                               int64_t ld_shared_scale, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                               int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                               int64_t batch_stride_scale, int fmt, const int32_t* kv_lens, const uint8_t* own_block,
                                               int64_t ld_own_block, int64_t shared_len, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                                               int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace,
                                               int64_t workspace_floats, void* stream) {
    return impl_f8(q, ld_q, k_shared, v_shared, ld_shared_bytes, k_shared_scale, v_shared_scale, ld_shared_scale, k_cache, v_cache, ld_kv_bytes,
                   batch_stride_kv_bytes, k_scale, v_scale, ld_scale, batch_stride_scale, fmt, kv_lens, 1, own_block, ld_own_block, 1, shared_len,
                   max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

// What attn_extend.hip and attn_extend_shared.hip share on top of attn2.h.  Device: the Q fragment and the accumulators of a lane, the K / V
// tile mover (bf16 and e4m3 cache), one 64-key step of the "swapped" online softmax (S^T = K Q^T, O^T += V^T P^T, log2 domain, deferred
// rescale), the double-buffered walk over a run of 64-key tiles, the store of a partial record and the fold of the partials of a row.  Host:
// the rule that deals the key tiles to runs, the padded head size, the dispatch over (e4m3, padded head size) and the refusals every entry
// point has.
#pragma once
#include "attn2.h"
#include <algorithm>
#include <type_traits>

namespace attn_tile {
using namespace attn2;

// The key runs of a launch (host): `ktiles` 64-key tiles are dealt to nsplit workgroups in contiguous runs of tps tiles.  One run while the
// nwg workgroups without a split give every other CU one; else enough runs of >= 4 tiles to reach about one workgroup per CU.
inline void key_runs(int64_t nwg, int ktiles, int& nsplit, int& tps) {
    int ns = 1;
    if (nwg < 128) ns = (int)std::min<int64_t>(std::max(1, ktiles / 4), (256 + nwg - 1) / nwg);
    ns = std::min(ns, 64);
    tps = (ktiles + ns - 1) / ns;
    nsplit = (ktiles + tps - 1) / tps;
}

inline int pick_dp(int64_t d) { return d <= 64 ? 64 : (d <= 96 ? 96 : 128); }      // the padded head size the kernels are built for

// launch(DP, F8) as compile-time constants for a cache of eb bytes per element and head size d: `launch` is a generic lambda that reads
// decltype(dp)::value and decltype(f8)::value
template <class Launch>
int dispatch(int eb, int64_t d, Launch&& launch) {
    using std::integral_constant;
    using std::bool_constant;
    const int dp = pick_dp(d);
    if (eb == 2) {
        switch (dp) {
            case 64: return launch(integral_constant<int, 64>{}, bool_constant<false>{});
            case 96: return launch(integral_constant<int, 96>{}, bool_constant<false>{});
            default: return launch(integral_constant<int, 128>{}, bool_constant<false>{});
        }
    }
    switch (dp) {
        case 64: return launch(integral_constant<int, 64>{}, bool_constant<true>{});
        case 96: return launch(integral_constant<int, 96>{}, bool_constant<true>{});
        default: return launch(integral_constant<int, 128>{}, bool_constant<true>{});
    }
}

// K / V rows as an entry point hands them over: row and block strides in BYTES (one block: bs 0), the e4m3 form with its scales [rows][Hkv]
// and their strides
struct CacheRef { const void* k; const void* v; int64_t ld, bs; const float* ks; const float* vs; int64_t ld_sc, bs_sc; };

// The refusals every entry point has, after its own (`shape_ok`: the lengths array, the counts and their limits, Hq % Hkv == 0): NULL
// pointers, d, q / o alignment and leading dimensions, cache and scale alignment by element width eb (2: bf16, 1: e4m3), the GQA group.
// `shared` is the second set of rows of the shared-prefix forms, or NULL.
inline int refuse(bool shape_ok, const void* q, int64_t ld_q, const void* o, int64_t ld_o, const CacheRef& own, const CacheRef* shared, int eb,
                  int64_t Hq, int64_t Hkv, int64_t d) {
    if (!shape_ok || !q || !o || !own.k || !own.v || (shared && (!shared->k || !shared->v))) return MM355_EINVAL;
    if ((d & 7) || d > 128) return MM355_EUNSUPPORTED;
    if (!mm_aligned16(q) || !mm_aligned16(o) || (ld_q & 7) || (ld_o & 7) || ld_q < Hq * d || ld_o < Hq * d) return MM355_EINVAL;
    const uintptr_t amask = eb == 2 ? 15u : 7u;              // one 16-byte (bf16) or 8-byte (e4m3) load per 8 columns
    for (const CacheRef* c : {&own, shared}) {
        if (!c) continue;
        if ((((uintptr_t)c->k | (uintptr_t)c->v) & amask) || ((c->ld | c->bs) & (int64_t)amask) || c->ld < Hkv * d * eb) return MM355_EINVAL;
        if (eb == 1 && (((((uintptr_t)c->ks) | ((uintptr_t)c->vs)) & 3u) || c->ld_sc < Hkv)) return MM355_EINVAL;
    }
    const int64_t G = Hq / Hkv;
    if (G != 1 && G != 2 && G != 4 && G != 8) return MM355_EUNSUPPORTED;      // GQA group sizes 1, 2, 4, 8
    return MM355_OK;
}

template <int DP> constexpr int tile_nv = (Geo<DP>::V64 + NT - 1) / NT;        // 16-byte vectors of a 64-row tile per thread

// chunk kk of this lane's Q fragment (the B operand: Q[row = fr][d chunk]) from its query row and head at qp; columns >= d are zero.  (The
// loop over the chunks stays in the kernels: as one function over the whole fragment it costs the d = 96 kernels an occupancy step.)
MM_DEV bf16x8 load_q(const uint16_t* qp, int kk, int d, int fq) {
    const int c = kk * 32 + fq * 8;
    return (c < d) ? *(const bf16x8*)(qp + c) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
}
// no key seen yet: O^T[d = j*16 + fq*4 + r][row = fr] = 0, running maximum -inf, sum 0
template <int DP>
MM_DEV void init_acc(f32x4 (&ot)[Geo<DP>::NF], float& m_run, float& l_run) {
    m_run = -INFINITY; l_run = 0.f;
#pragma unroll
    for (int j = 0; j < Geo<DP>::NF; ++j) ot[j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

template <int NV, bool F8> struct Stage;
template <int NV> struct Stage<NV, false> { u32x4 r[NV]; };
template <int NV> struct Stage<NV, true> { u32x2 r[NV]; float s[NV]; };

// rows [row0, row0 + 64) of one KV head -> registers; rows past `end` repeat row end - 1 (masked by the caller), columns >= d are zero
template <int DP, int NV, bool F8>
MM_DEV void load_tile(Stage<NV, F8>& st, const unsigned char* base, const float* sbase, int64_t ld, int64_t ld_sc, int row0, int end, int d, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * NT, row = v / (DP / 8), c = v % (DP / 8);
        const bool on = v < Geo<DP>::V64 && c * 8 < d;
        const int rr = min(row0 + row, end - 1);
        if constexpr (F8) {
            st.r[i] = on ? *(const u32x2*)(base + (int64_t)rr * ld + c * 8) : u32x2{0u, 0u};
            st.s[i] = on ? sbase[(int64_t)rr * ld_sc] : 0.f;
        } else {
            st.r[i] = on ? *(const u32x4*)(base + (int64_t)rr * ld + c * 16) : u32x4{0u, 0u, 0u, 0u};
        }
    }
}
// The block numbers of the rows load_tile_idx is about to move: blk[i] = tbl[row - first] of this thread's i-th vector, clamped into [0, nblk)
// (an entry is the caller's promise; a wrong one still names a block of the cache) and the column into [0, cols).  Rows are clamped as
// load_tile clamps them, so no entry at or beyond end - first is read; a tile that starts at or beyond `end` reads nothing.
template <int DP, int NV>
MM_DEV void load_blocks(int (&blk)[NV], const uint8_t* tbl, int cols, int nblk, int first, int row0, int end, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * NT, row = v / (DP / 8);
        const bool on = v < Geo<DP>::V64 && row0 < end;
        const int col = min(min(row0 + row, end - 1) - first, cols - 1);
        blk[i] = on ? min((int)tbl[col], nblk - 1) : 0;
    }
}
// load_tile where row r of the tile lives in block blk[] of a [blocks][rows] cache (block strides bs BYTES / bs_sc scales): the same
// loads from other addresses, so the tile in LDS -- and everything computed from it -- is load_tile's on the gathered rows
template <int DP, int NV, bool F8>
MM_DEV void load_tile_idx(Stage<NV, F8>& st, const unsigned char* base, const float* sbase, int64_t ld, int64_t ld_sc, int64_t bs, int64_t bs_sc,
                          const int (&blk)[NV], int row0, int end, int d, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * NT, row = v / (DP / 8), c = v % (DP / 8);
        const bool on = v < Geo<DP>::V64 && c * 8 < d;
        const int rr = min(row0 + row, end - 1);
        const unsigned char* p = base + blk[i] * bs + (int64_t)rr * ld;
        if constexpr (F8) {
            st.r[i] = on ? *(const u32x2*)(p + c * 8) : u32x2{0u, 0u};
            st.s[i] = on ? sbase[blk[i] * bs_sc + (int64_t)rr * ld_sc] : 0.f;
        } else {
            st.r[i] = on ? *(const u32x4*)(p + c * 16) : u32x4{0u, 0u, 0u, 0u};
        }
    }
}
template <int DP, int NV, bool F8>
MM_DEV void store_tile(const Stage<NV, F8>& st, unsigned char* s, int tid) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * NT, row = v / (DP / 8), c = v % (DP / 8);
        if (v >= Geo<DP>::V64) continue;
        u32x4 w;
        if constexpr (F8) {                                  // e4m3 -> fp32 is exact, times a power of two is exact and a bf16 value
            const mm_f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)st.r[i].x, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)st.r[i].x, true);
            const mm_f32x2 e = __builtin_amdgcn_cvt_pk_f32_fp8((int)st.r[i].y, false), f = __builtin_amdgcn_cvt_pk_f32_fp8((int)st.r[i].y, true);
            const float sc = st.s[i];
            w.x = pack2bf(a.x * sc, a.y * sc); w.y = pack2bf(b.x * sc, b.y * sc);
            w.z = pack2bf(e.x * sc, e.y * sc); w.w = pack2bf(f.x * sc, f.y * sc);
        } else {
            w = st.r[i];
        }
        *(u32x4*)(s + offN<Geo<DP>::DS>(row, c)) = w;
    }
}

// One wave, 16 packed rows (lane's row = fr), the 64 keys [kv0, kv0 + 64) in sK / sV: scores, mask (key > klim of the lane's row, looked at
// only when `ragged`), running maximum m_run (log2 domain) with deferred rescale, sum l_run, O^T accumulators ot.
template <int DP>
MM_DEV void softmax_tile(const unsigned char* sK, const unsigned char* sV, const bf16x8 (&qf)[Geo<DP>::KS], f32x4 (&ot)[Geo<DP>::NF], float& m_run,
                         float& l_run, int kv0, bool ragged, int klim, float sl2, int fr, int fq) {
    constexpr int DS = Geo<DP>::DS, KS = Geo<DP>::KS, NF = Geo<DP>::NF;
    constexpr float RESCALE_THR = 6.0f;                      // log2 units: keep the old running max while it grows < 2^6
    f32x4 st[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const bf16x8 kf = *(const bf16x8*)(sK + offN<DS>(j * 16 + fr, kk * 4 + fq));
            st[j] = mfma16(kf, qf[kk], st[j]);
        }
    if (ragged) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (kv0 + j * 16 + fq * 4 + r > klim) st[j][r] = -INFINITY;
    }
    float mx = -INFINITY;                                    // max of the RAW scores (scale > 0 commutes with max)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[j][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    mx *= sl2;
    // deferred rescale: move the running max (and touch the O accumulators) only when some row's max grew by more than 2^THR
    const bool grow = mx > m_run + RESCALE_THR || m_run == -INFINITY;
    if (__any(grow && mx > -INFINITY)) {
        const float mn = fmaxf(m_run, mx);
        const float alpha = (m_run == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(m_run - mn);
        l_run *= alpha;
#pragma unroll
        for (int j = 0; j < NF; ++j) ot[j] *= alpha;
        m_run = mn;
    }
    const float mref = m_run;
    float rs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = (mref == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(fmaf(st[j][r], sl2, -mref));
            st[j][r] = p;
            rs += p;
        }
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    l_run += rs;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 pb = pack_acc(st[2 * kk], st[2 * kk + 1]);
#pragma unroll
        for (int j = 0; j < NF; ++j) {
            const bf16x8 va = read_nat_perm<DS>(sV, kk * 32, j, fr, fq);      // V^T[d][keys perm]
            ot[j] = mfma16(va, pb, ot[j]);
        }
    }
}

// The workgroup's walk over the ntiles 64-key tiles from key k_lo, double buffered: fetch(rk, rv, row0, end) moves the K and V tiles at row0
// into registers, clamping its rows at `end` (load_tile's rule; the indexed form plugs in here), while the waves run softmax_tile on the tile
// in sK / sV.  A wave takes part in a tile while it is `wave_on` and the tile starts at or before wave_hi, the largest key limit of its rows;
// the per-lane mask (key > klim) is looked at only in tiles that reach beyond wave_lo, the smallest one.  All threads of the workgroup call.
template <int DP, bool F8, class Fetch>
MM_DEV void walk_tiles(Fetch&& fetch, unsigned char* sK, unsigned char* sV, const bf16x8 (&qf)[Geo<DP>::KS], f32x4 (&ot)[Geo<DP>::NF],
                       float& m_run, float& l_run, int k_lo, int ntiles, int end, bool wave_on, int wave_lo, int wave_hi, int klim, float sl2,
                       int tid, int fr, int fq) {
    constexpr int NV = tile_nv<DP>;
    if (ntiles <= 0) return;
    Stage<NV, F8> rk, rv;
    fetch(rk, rv, k_lo, end);
    store_tile<DP, NV, F8>(rk, sK, tid);
    store_tile<DP, NV, F8>(rv, sV, tid);
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const int kv0 = k_lo + t * 64;
        const bool more = t + 1 < ntiles;
        if (more) fetch(rk, rv, kv0 + 64, end);
        if (wave_on && kv0 <= wave_hi)                       // a wave whose rows all precede this tile has nothing to do here
            softmax_tile<DP>(sK, sV, qf, ot, m_run, l_run, kv0, kv0 + 63 > wave_lo, klim, sl2, fr, fq);
        __syncthreads();                                     // every wave is done reading this tile
        if (more) {
            store_tile<DP, NV, F8>(rk, sK, tid);
            store_tile<DP, NV, F8>(rv, sV, tid);
            __syncthreads();
        }
    }
}

// A lane's share of the partial record of packed row `row` in a workspace of `nrows` records: unnormalised fp32 O [nrows][DP], then the
// reference maximum (log2 domain) and the sum [nrows][2]
template <int DP>
MM_DEV void store_partial(float* ws, int64_t nrows, int64_t row, const f32x4 (&ot)[Geo<DP>::NF], float m_run, float l_run, int fq) {
    float* po = ws + row * DP;
#pragma unroll
    for (int j = 0; j < Geo<DP>::NF; ++j) *(f32x4*)(po + j * 16 + fq * 4) = ot[j];
    if (fq == 0) {
        float* ml = ws + nrows * DP + row * 2;
        ml[0] = m_run; ml[1] = l_run;
    }
}

// sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s over the `nslots` partials of one packed row, columns [c, c + 4): partial s has its O at
// po + (row0 + s * stride) * DP and its (m, l) at ml + (row0 + s * stride) * 2; a partial that saw no key has m = -inf
template <int DP>
MM_DEV u32x2 merge_partials(const float* po, const float* ml, int64_t row0, int64_t stride, int nslots, int c) {
    float M = -INFINITY;
    for (int s = 0; s < nslots; ++s) M = fmaxf(M, ml[(row0 + s * stride) * 2]);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float l = 0.f;
    for (int s = 0; s < nslots; ++s) {
        const int64_t row = row0 + s * stride;
        const float m = ml[row * 2];
        if (m == -INFINITY) continue;
        const float w = __builtin_amdgcn_exp2f(m - M);
        l += w * ml[row * 2 + 1];
        acc += w * *(const f32x4*)(po + row * DP + c);
    }
    const float inv = l > 0.f ? 1.0f / l : 0.f;
    u32x2 w;
    w.x = pack2bf(acc[0] * inv, acc[1] * inv);
    w.y = pack2bf(acc[2] * inv, acc[3] * inv);
    return w;
}
}  // namespace attn_tile

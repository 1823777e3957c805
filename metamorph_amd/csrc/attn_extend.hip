// Attention of n NEW rows against a filled KV cache (gfx950): row (b, i) sits at position past[b] + i and attends the cache rows
// [0, past[b] + i]; the chunk's own rows are already in the cache (the append comes first).  The shape between the prompt pass
// (mm355_attn_fwd: one length for queries and keys) and the decode step (mm355_attn_decode: one query row per sequence).
//
// The kernel is attn2.hip's fwd_kernel ("swapped" formulation: S^T = K Q^T, O^T += V^T P^T, natural [64][d] K / V tiles in LDS with the
// 16-B chunk swizzle, P never leaves registers, online softmax in the log2 domain with deferred rescale) with three changes:
//   * query rows are PACKED per KV head: packed row r = i * G + g is query row i of head hk * G + g (G = the GQA group), so a workgroup
//     (sequence, KV head, 64 packed rows = 16 per wave) reads every K / V tile once for the whole group, and n = 1 with G = 4 is 4 rows of
//     one fragment instead of 4 workgroups;
//   * the key limit is per row and comes from the device: key j is visible to row r iff j <= past[b] + r / G;
//   * when (sequences x KV heads x row tiles) is a handful of workgroups, the 64-key tiles are dealt to `nsplit` workgroups in contiguous
//     runs; each writes its unnormalised fp32 O, running reference maximum and sum, and extend_merge_kernel (a second launch) folds them.
//     The split depends on the launch arguments only (never on past[]), so the bf16 and the e4m3 form of one call split alike.
// The e4m3 form differs in the tile mover alone: 8 bytes per 8 columns plus the head-row's scale, widened to bf16 (exact: mm355.h, the
// KV8 contract) where the tile is written into LDS.  Everything after that is the same code on the same bits.
// Cache rows >= past[b] + n are never read: ragged tiles clamp their row index to the last visible row of the workgroup.
// The pieces of the kernel (Q fragment, tile mover, softmax step, tile walk, partial record and its fold) and of the host side (key runs,
// dispatch, common refusals) live in attn_tile.h, shared with attn_extend_shared.hip.
//
// The ragged form (RAG; mm355_attn_extend_ragged) is the same kernel with a row table: sequence b brings n_b = row_start[b + 1] - row_start[b]
// rows, packed at rows row_start[b] + i of q / o.  The launch is sized by the host bound n_max; n_b is clamped into [0, n_max], a row index
// into [0, q_rows), and a workgroup whose row tile lies beyond n_b * G leaves before it reads anything of its sequence.  The plan is a
// function of the launch arguments (n_max for n), so a uniform table runs the very workgroups of the plain form.
#include "attn_tile.h"

namespace {
using namespace attn_tile;

struct XArgs {
    const uint16_t* q; int64_t ld_q;
    const unsigned char* k; const unsigned char* v; int64_t ld_kv, bs_kv;      // BYTES per cache row / per sequence
    const float* ks; const float* vs; int64_t ld_sc, bs_sc;                    // e4m3 form: scales [B][rows][Hkv]
    const int32_t* past; uint16_t* o; int64_t ld_o; float* ws;
    const int32_t* row_start; int q_rows;                                      // ragged form: n below is n_max, R and nqt belong to it
    int n, Hkv, d, G, R, nqt, nsplit, tps, max_kv; int64_t rpad;
    float scale;
};

struct Plan { int G, R, nqt, nsplit, tps; int64_t rpad; };

// nsplit: 1 while the row tiles alone give every other CU a workgroup; else enough runs of >= 4 key tiles to reach about one per CU
Plan make_plan(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t max_kv_len) {
    Plan p;
    p.G = (int)(Hq / Hkv);
    p.R = (int)(n * p.G);
    p.nqt = (p.R + 63) / 64;
    p.rpad = (int64_t)p.nqt * 64;
    const int64_t nwg = B * Hkv * p.nqt;
    key_runs(nwg, (int)((max_kv_len + 63) / 64), p.nsplit, p.tps);
    return p;
}

// the rows of sequence b in the ragged form: n_b clamped into [0, n_max]; first = row_start[b]
MM_DEV int ragged_rows(const XArgs& a, int b, int& first) {
    first = a.row_start[b];
    return (int)min(max((int64_t)a.row_start[b + 1] - first, (int64_t)0), (int64_t)a.n);
}
// row i of sequence b in q / o: b * n + i, or the table's row clamped into [0, q_rows)
template <bool RAG>
MM_DEV int64_t seq_row(const XArgs& a, int b, int n, int first, int i) {
    if constexpr (RAG) return min(max((int64_t)first + i, (int64_t)0), (int64_t)a.q_rows - 1);
    else return (int64_t)b * n + i;
}

template <int DP, bool F8, bool RAG>
__global__ __launch_bounds__(NT) void extend_kernel(XArgs a) {
    using G_ = Geo<DP>;
    constexpr int KS = G_::KS, NF = G_::NF, NV = tile_nv<DP>;
    constexpr int EPI = 4 * 16 * DP * 2;                    // bf16 output staging
    constexpr int SMEM = 2 * G_::T64 > EPI ? 2 * G_::T64 : EPI;
    __shared__ __attribute__((aligned(16))) unsigned char smem[SMEM];
    unsigned char* sK = smem;
    unsigned char* sV = smem + G_::T64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int qt = blockIdx.x / a.nsplit, split = blockIdx.x % a.nsplit;
    const int hk = blockIdx.y, b = blockIdx.z;
    const int d = a.d, G = a.G;
    const int q0 = qt * 64, qw0 = q0 + wave * 16;
    int R = a.R, n = a.n, first = 0;
    if constexpr (RAG) {
        n = ragged_rows(a, b, first);
        R = n * G;
        if (q0 >= R) return;                                 // (the whole workgroup: an empty sequence, a tile beyond its rows)
    }
    const int past = a.past[b];
    // last key (exclusive) any row of this workgroup sees; the host bound keeps a wrong past[] inside the cache
    const int kv_end = min(past + min(R - 1, q0 + 63) / G + 1, a.max_kv);
    const int ntiles = (kv_end + 63) >> 6;
    const int t0 = split * a.tps, t1 = min(ntiles, t0 + a.tps);

    const int pr = min(qw0 + fr, R - 1);                     // this lane's packed row (clamped: rows >= R are not stored)
    const int qi = pr / G, qg = pr - qi * G;
    const int klim = past + qi;                              // last visible key of the row
    const int wave_lo = past + min(qw0, R - 1) / G, wave_hi = past + min(qw0 + 15, R - 1) / G;
    const bool wave_on = qw0 < R;

    bf16x8 qf[KS];
    {
        const uint16_t* qp = a.q + seq_row<RAG>(a, b, n, first, qi) * a.ld_q + (int64_t)(hk * G + qg) * d;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) qf[kk] = load_q(qp, kk, d, fq);
    }
    f32x4 ot[NF];
    float m_run, l_run;
    init_acc<DP>(ot, m_run, l_run);

    constexpr int EB = F8 ? 1 : 2;
    const unsigned char* kbase = a.k + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
    const unsigned char* vbase = a.v + (int64_t)b * a.bs_kv + (int64_t)hk * d * EB;
    const float* ksb = F8 ? a.ks + (int64_t)b * a.bs_sc + hk : nullptr;
    const float* vsb = F8 ? a.vs + (int64_t)b * a.bs_sc + hk : nullptr;
    const float sl2 = a.scale * 1.4426950408889634f;         // scores in log2 domain: exp2(s*sl2 - m), the scale on the fp32 side

    // the run's tiles; loads clamp at the workgroup's kv_end, not at the run's end
    auto fetch = [&](Stage<NV, F8>& rk, Stage<NV, F8>& rv, int row0, int end) {
        load_tile<DP, NV, F8>(rk, kbase, ksb, a.ld_kv, a.ld_sc, row0, end, d, tid);
        load_tile<DP, NV, F8>(rv, vbase, vsb, a.ld_kv, a.ld_sc, row0, end, d, tid);
    };
    walk_tiles<DP, F8>(fetch, sK, sV, qf, ot, m_run, l_run, t0 * 64, t1 - t0, kv_end, wave_on, wave_lo, wave_hi, klim, sl2, tid, fr, fq);

    if (a.nsplit > 1) {                                      // partial: unnormalised O, reference maximum (log2 domain) and sum
        if (qw0 + fr < R)
            store_partial<DP>(a.ws, (int64_t)gridDim.z * a.Hkv * a.nsplit * a.rpad, (((int64_t)b * a.Hkv + hk) * a.nsplit + split) * a.rpad + qw0 + fr,
                              ot, m_run, l_run, fq);
        return;
    }
    // epilogue: O = O^T / l -> bf16 [row][d] in LDS -> row-contiguous 16-B stores
    unsigned char* so = smem + wave * (16 * DP * 2);
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        u32x2 w;
        w.x = pack2bf(ot[j][0] * inv, ot[j][1] * inv);
        w.y = pack2bf(ot[j][2] * inv, ot[j][3] * inv);
        *(u32x2*)(so + fr * (DP * 2) + (j * 16 + fq * 4) * 2) = w;
    }
    __syncthreads();
    for (int v = lane; v < 16 * (d >> 3); v += 64) {
        const int r = v / (d >> 3), c = (v % (d >> 3)) * 8;
        const int p = qw0 + r;
        if (p < R) {
            const int i = p / G, g = p - i * G;
            *(u32x4*)(a.o + seq_row<RAG>(a, b, n, first, i) * a.ld_o + (int64_t)(hk * G + g) * d + c) = *(const u32x4*)(so + r * (DP * 2) + c * 2);
        }
    }
}

// o[row][4 columns] = sum_s 2^(m_s - M) O_s / sum_s 2^(m_s - M) l_s over the key runs of one packed row; a run that saw no key has m = -inf
template <int DP, bool RAG>
__global__ __launch_bounds__(NT) void extend_merge_kernel(XArgs a) {
    const int hk = blockIdx.y, b = blockIdx.z;
    const int idx = blockIdx.x * NT + threadIdx.x;
    const int p = idx / (DP / 4), c = (idx % (DP / 4)) * 4;
    int R = a.R, n = a.n, first = 0;
    if constexpr (RAG) {                                     // the rows the first launch skipped have no partials
        n = ragged_rows(a, b, first);
        R = n * a.G;
    }
    if (p >= R || c >= a.d) return;
    const int64_t row0 = ((int64_t)b * a.Hkv + hk) * a.nsplit * a.rpad + p;
    const float* ml = a.ws + (int64_t)gridDim.z * a.Hkv * a.nsplit * a.rpad * DP;
    const u32x2 w = merge_partials<DP>(a.ws, ml, row0, a.rpad, a.nsplit, c);
    const int i = p / a.G, g = p - i * a.G;
    *(u32x2*)(a.o + seq_row<RAG>(a, b, n, first, i) * a.ld_o + (int64_t)(hk * a.G + g) * a.d + c) = w;
}

template <int DP, bool F8, bool RAG>
int launch(const XArgs& a, int64_t B, hipStream_t s) {
    hipLaunchKernelGGL((extend_kernel<DP, F8, RAG>), dim3((unsigned)(a.nqt * a.nsplit), (unsigned)a.Hkv, (unsigned)B), dim3(NT), 0, s, a);
    if (a.nsplit > 1) {
        if (mm_launch_status() != MM355_OK) return MM355_ELAUNCH;
        const unsigned gx = (unsigned)(((int64_t)a.R * (DP / 4) + NT - 1) / NT);
        hipLaunchKernelGGL((extend_merge_kernel<DP, RAG>), dim3(gx, (unsigned)a.Hkv, (unsigned)B), dim3(NT), 0, s, a);
    }
    return mm_launch_status();
}

// eb = bytes per cached element (2: bf16, 1: e4m3); ld_kv / bs_kv arrive in BYTES.  row_start: the ragged form's table (then n is n_max and
// q_rows the rows of q / o), NULL for the plain form
int extend_impl(const mm355_bf16* q, int64_t ld_q, const void* k, const void* v, int64_t ld_kv, int64_t bs_kv, int eb, const float* ks,
                const float* vs, int64_t ld_sc, int64_t bs_sc, const int32_t* past, const int32_t* row_start, int64_t n, int64_t q_rows, int64_t max_kv_len,
                mm355_bf16* o, int64_t ld_o,
                int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* ws, int64_t ws_floats, void* stream) {
    const CacheRef own{k, v, ld_kv, bs_kv, ks, vs, ld_sc, bs_sc};
    const bool shape_ok = past && B > 0 && n > 0 && Hq > 0 && Hkv > 0 && !(Hq % Hkv) && d > 0 && max_kv_len > 0 && n <= max_kv_len &&
                          max_kv_len <= 0x7fffffc0ll && n * (Hq / Hkv) <= 0x7fffffc0ll && B <= 65535 && Hkv <= 65535 && q_rows <= 0x7fffffffll;
    if (const int rc = refuse(shape_ok, q, ld_q, o, ld_o, own, nullptr, eb, Hq, Hkv, d)) return rc;
    const Plan p = make_plan(B, n, Hq, Hkv, max_kv_len);
    if (p.nsplit > 1 && (!ws || (((uintptr_t)ws) & 15u) || ws_floats < B * Hkv * p.nsplit * p.rpad * (pick_dp(d) + 2))) return MM355_EINVAL;
    XArgs a{q, ld_q, (const unsigned char*)k, (const unsigned char*)v, ld_kv, bs_kv, ks, vs, ld_sc, bs_sc, past, o, ld_o, ws, row_start, (int)q_rows,
            (int)n, (int)Hkv, (int)d, p.G, p.R, p.nqt, p.nsplit, p.tps, (int)max_kv_len, p.rpad, scale};
    return dispatch(eb, d, [&](auto dp_, auto f8_) {
        constexpr int DP = decltype(dp_)::value;
        constexpr bool F8 = decltype(f8_)::value;
        return row_start ? launch<DP, F8, true>(a, B, (hipStream_t)stream) : launch<DP, F8, false>(a, B, (hipStream_t)stream);
    });
}

}  // namespace

extern "C" int64_t mm355_attn_extend_ws_floats(int64_t B, int64_t n, int64_t Hq, int64_t Hkv, int64_t d, int64_t max_kv_len) {
    if (B <= 0 || n <= 0 || Hq <= 0 || Hkv <= 0 || (Hq % Hkv) || d <= 0 || d > 128 || max_kv_len <= 0) return 0;
    const Plan p = make_plan(B, n, Hq, Hkv, max_kv_len);
    return p.nsplit > 1 ? B * Hkv * p.nsplit * p.rpad * (pick_dp(d) + 2) : 0;
}

extern "C" int mm355_attn_extend(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                 int64_t batch_stride_kv, const int32_t* past, int64_t n, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o,
                                 int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace, int64_t workspace_floats,
                                 void* stream) {
    (void)hipGetLastError();
    return extend_impl(q, ld_q, k_cache, v_cache, ld_kv * 2, batch_stride_kv * 2, 2, nullptr, nullptr, 0, 0, past, nullptr, n, 0, max_kv_len, o, ld_o, B,
                       Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_extend_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                    int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                    int64_t batch_stride_scale, int fmt, const int32_t* past, int64_t n, int64_t max_kv_len, mm355_bf16* o,
                                    int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale, float* workspace,
                                    int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !k_scale || !v_scale) return MM355_EINVAL;
    return extend_impl(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, 1, k_scale, v_scale, ld_scale, batch_stride_scale, past, nullptr, n,
                       0, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int64_t mm355_attn_extend_ragged_ws_floats(int64_t B, int64_t n_max, int64_t Hq, int64_t Hkv, int64_t d, int64_t max_kv_len) {
    return mm355_attn_extend_ws_floats(B, n_max, Hq, Hkv, d, max_kv_len);
}

extern "C" int mm355_attn_extend_ragged(const mm355_bf16* q, int64_t ld_q, const mm355_bf16* k_cache, const mm355_bf16* v_cache, int64_t ld_kv,
                                        int64_t batch_stride_kv, const int32_t* past, const int32_t* row_start, int64_t n_max, int64_t q_rows,
                                        int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv, int64_t d, float scale,
                                        float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (!row_start || n_max < 1 || q_rows < 1) return MM355_EINVAL;
    return extend_impl(q, ld_q, k_cache, v_cache, ld_kv * 2, batch_stride_kv * 2, 2, nullptr, nullptr, 0, 0, past, row_start, n_max, q_rows, max_kv_len,
                       o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

extern "C" int mm355_attn_extend_ragged_f8(const mm355_bf16* q, int64_t ld_q, const uint8_t* k_cache, const uint8_t* v_cache, int64_t ld_kv_bytes,
                                           int64_t batch_stride_kv_bytes, const float* k_scale, const float* v_scale, int64_t ld_scale,
                                           int64_t batch_stride_scale, int fmt, const int32_t* past, const int32_t* row_start, int64_t n_max,
                                           int64_t q_rows, int64_t max_kv_len, mm355_bf16* o, int64_t ld_o, int64_t B, int64_t Hq, int64_t Hkv,
                                           int64_t d, float scale, float* workspace, int64_t workspace_floats, void* stream) {
    (void)hipGetLastError();
    if (fmt != MM355_KV8_E4M3 || !k_scale || !v_scale || !row_start || n_max < 1 || q_rows < 1) return MM355_EINVAL;
    return extend_impl(q, ld_q, k_cache, v_cache, ld_kv_bytes, batch_stride_kv_bytes, 1, k_scale, v_scale, ld_scale, batch_stride_scale, past,
                       row_start, n_max, q_rows, max_kv_len, o, ld_o, B, Hq, Hkv, d, scale, workspace, workspace_floats, stream);
}

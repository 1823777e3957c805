// Beam search in the device token loop (functional.BeamLoopGraph): HF's GenerationMixin._beam_search for one prompt, greedy, without
// logits processors.  Two entry points stand where the argmax and mm355_greedy_advance stand in the greedy loop:
//   mm355_beam_select_rows_f32: the log-softmax statistics of the K logits rows and the M best of the K * V accumulated scores, sorted;
//   mm355_beam_advance:         HF's bookkeeping on those M candidates (running beams, finished pool, stopping rule), the back-pointer
//                               logs, the table of own cache rows for mm355_attn_decode_shared_idx and the next input rows.
// The host-side models, which the kernels equal bit for bit, are metamorph_amd.functional.beam_select_host and beam_step_host.
#include "argrows.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int BM_NT = 1024;
constexpr int BM_MAXM = 9 * MM355_BEAM_MAX;                  // candidates: max(2, 1 + eos ids) * K
constexpr int BM_LIST = 2048;                                // a row's survivors of the first filter kept in LDS

// order-preserving key of a float that is no NaN (sample.hip's): a < b <=> okey(a) < okey(b); -0 and +0 share a key
MM_DEV uint32_t okey(float x) {
    const uint32_t b = __float_as_uint(x + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
MM_DEV float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The order of the candidates: value descending, a NaN after every number, among equals (and among NaNs) the lower index first.  A total
// order on (value, index) pairs with distinct indices, so a rank is a function of the set alone.
MM_DEV bool cand_beats(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return bn;
    if (an) return ai < bi;
    return av > bv || (av == bv && ai < bi);
}

// (value key, column) as one 64-bit key whose descending order is cand_beats' on numbers: distinct columns make the keys distinct
MM_DEV uint64_t key64(uint32_t k, int col) { return ((uint64_t)k << 32) | (uint32_t)(0x7fffffff - col); }

// one count into a 256-bin LDS histogram; lanes of a wave that all hit one bin (rows of equal scores) add once
MM_DEV void hist_add(uint32_t* h, int d) {
    const unsigned long long act = __ballot(1);
    const int d0 = __builtin_amdgcn_readfirstlane(d);
    if (__ballot(d == d0) == act) {
        if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&h[d0], (uint32_t)__popcll(act));
    } else {
        atomicAdd(&h[d], 1u);
    }
}

// wave 0: the highest bin b whose bins b .. 255 together hold >= need, and what is left of need inside that bin (integers: any order)
MM_DEV void find_bin(const uint32_t* h, uint32_t need, uint32_t* s_out) {
    const int l = threadIdx.x;
    uint32_t b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = h[4 * l + j];
    const uint32_t s = b[0] + b[1] + b[2] + b[3];
    uint32_t suf = s;                                        // -> the sum over the bins of lanes l .. 63
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_down((int)suf, o, 64);
        if (l + o < 64) suf += t;
    }
    const unsigned long long mask = __ballot(suf >= need);
    const int sel = mask ? 63 - __clzll((long long)mask) : 0;
    if (l == sel) {
        uint32_t acc = suf - s;
        int bin = 4 * l;
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            if (acc + b[j] >= need) { bin = 4 * l + j; break; }
            acc += b[j];
        }
        s_out[0] = (uint32_t)bin;
        s_out[1] = need > acc ? need - acc : 1u;
    }
}

// The need-th largest of the distinct 64-bit keys for_each(f) hands to f (every thread of the workgroup calls select64; for_each gives a
// thread its share): eight rounds of 256 bins from the top byte down, integer LDS atomics only.
template <class ForEach>
MM_DEV uint64_t select64(ForEach for_each, uint32_t need, uint32_t* h, uint32_t* s_out) {
    uint64_t prefix = 0;
    for (int r = 0; r < 8; ++r) {
        const int sh = 56 - 8 * r;
        __syncthreads();
        if (threadIdx.x < 256) h[threadIdx.x] = 0;
        __syncthreads();
        for_each([&](uint64_t k) {
            if (r == 0 || (k >> (sh + 8)) == (prefix >> (sh + 8))) hist_add(h, (int)((k >> sh) & 255));
        });
        __syncthreads();
        if (threadIdx.x < 64) find_bin(h, need, s_out);
        __syncthreads();
        prefix |= (uint64_t)s_out[0] << sh;
        need = s_out[1];
    }
    return prefix;
}

// stage 1, one workgroup per row b: stats[b] = (m, lse) as token_note_kernel computes them, and the row's min(M, V) best accumulated
// scores acc_i = ((x_i - m) - lse) + running[b] with their flat indices b * V + i, in any order, into part[b][0 .. Mr).
// acc is non-decreasing in x, so thread t's best acc is that of its largest x: the Mr-th largest of the 1024 thread maxima bounds the
// row's Mr-th largest from below, and only what reaches it (a few hundred columns of a row of logits) enters the exact select.
__global__ __launch_bounds__(BM_NT) void beam_rows_kernel(const float* __restrict__ x, int V, const float* __restrict__ running, int M,
                                                          float* __restrict__ stats, float* __restrict__ part_val, int* __restrict__ part_idx) {
    __shared__ float red[BM_NT / 64];
    __shared__ uint32_t h[256], s_out[2];
    __shared__ uint64_t s_list[BM_LIST];
    __shared__ int s_n, s_c;
    const int b = blockIdx.x, Mr = min(M, V);
    const float* row = x + (int64_t)b * V;
    float* pv = part_val + (int64_t)b * M;
    int* pi = part_idx + (int64_t)b * M;

    float tm = -INFINITY, nan = 0.f;                         // (fmaxf drops NaNs: they are counted beside the maximum)
    row_for_cols<BM_NT>(row, V, [&](float v, int) {
        tm = fmaxf(tm, v);
        if (v != v) nan = 1.f;
    });
    const float m = block_max<BM_NT>(tm, red);
    nan = block_max<BM_NT>(nan, red);
    if (nan != 0.f || !(fabsf(m) < INFINITY)) {              // NaN, +inf, or a row of -inf only: every score of the row is NaN
        if (threadIdx.x == 0) { stats[2 * b] = m; stats[2 * b + 1] = __builtin_nanf(""); }
        for (int i = threadIdx.x; i < Mr; i += BM_NT) { pv[i] = __builtin_nanf(""); pi[i] = b * V + i; }
        return;
    }
    // the sum as token_note_kernel's fixed tree: thread t adds the columns t, t + 1024, ... in that order, then wave butterflies, 16 waves
    float acc = 0.f;
    row_for_cols<BM_NT>(row, V, [&](float v, int) { acc += __expf(v - m); });
    const float lse = logf(block_sum<BM_NT>(acc, red));
    const float run = running[b];
    if (threadIdx.x == 0) { stats[2 * b] = m; stats[2 * b + 1] = lse; }
    auto score = [&](float v) { return ((v - m) - lse) + run; };

    // the lower bound: the Mr-th largest thread maximum (a thread without a column holds -inf, which bounds nothing)
    const uint64_t tkey = key64(okey(score(tm)), (int)threadIdx.x);
    const uint32_t key0 = (uint32_t)(select64([&](auto f) { f(tkey); }, (uint32_t)Mr, h, s_out) >> 32);

    if (threadIdx.x == 0) { s_n = 0; s_c = 0; }
    __syncthreads();
    row_for_cols<BM_NT>(row, V, [&](float v, int c) {
        const uint32_t k = okey(score(v));
        if (k >= key0) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < BM_LIST) s_list[slot] = key64(k, c);
        }
    });
    __syncthreads();
    const int n = s_n;
    // the survivors' keys: from the list (its order is arbitrary, the integer counts do not see it), or from the row again where rows of
    // near-equal scores (every beam but the first in step 0, whose -1e9 swallows the differences) overflow it
    auto survivors = [&](auto f) {
        if (n <= BM_LIST) {
            for (int i = threadIdx.x; i < n; i += BM_NT) f(s_list[i]);
        } else {
            row_for_cols<BM_NT>(row, V, [&](float v, int c) {
                const uint32_t k = okey(score(v));
                if (k >= key0) f(key64(k, c));
            });
        }
    };
    const uint64_t t64 = select64(survivors, (uint32_t)Mr, h, s_out);
    survivors([&](uint64_t k) {                                // exactly Mr keys reach t64
        if (k >= t64) {
            const int slot = atomicAdd(&s_c, 1);
            if (slot < Mr) {
                pv[slot] = okey_inv((uint32_t)(k >> 32));
                pi[slot] = b * V + (0x7fffffff - (int)(uint32_t)k);
            }
        }
    });
}

// stage 2, one workgroup: the rank of each of the K * Mr partial candidates among all of them; ranks below M are the output, in order
__global__ __launch_bounds__(BM_NT) void beam_merge_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx, int K, int M,
                                                           int Mr, float* __restrict__ cand_val, int* __restrict__ cand_idx) {
    __shared__ float sv[MM355_BEAM_MAX * BM_MAXM];
    __shared__ int si[MM355_BEAM_MAX * BM_MAXM];
    const int n = K * Mr;
    for (int i = threadIdx.x; i < n; i += BM_NT) {
        const int b = i / Mr, j = i - b * Mr;
        sv[i] = part_val[(int64_t)b * M + j];
        si[i] = part_idx[(int64_t)b * M + j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += BM_NT) {
        const float v = sv[i];
        const int id = si[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += cand_beats(sv[j], si[j], v, id) ? 1 : 0;
        if (rank < M) { cand_val[rank] = v; cand_idx[rank] = id; }
    }
}

struct AdvanceArgs {
    const float* cand_val; const int* cand_idx;
    int K, M, V;
    float *running, *fin_score;
    int *fin_flag, *fin_end, *scal, *live, *tok, *parent, *tok_log, *parent_log;
    uint8_t* own_block; int64_t ld_ob;
    const uint16_t* embed; int64_t ld_embed;
    uint16_t* x_in; int64_t ld_x; int h;
    const float* len_pow;
    int max_new_tokens, early_stopping, fixed_len, n_eos;
    int eos[MM355_GREEDY_MAX_EOS];
};

constexpr float BM_NEG = -1.0e9f;

// one workgroup: thread 0 runs HF's bookkeeping on the M candidates (functional.beam_step_host, steps 2 - 6), then every thread copies
__global__ __launch_bounds__(256) void beam_advance_kernel(const AdvanceArgs a) {
    __shared__ float s_val[BM_MAXM], s_ms[MM355_BEAM_MAX + BM_MAXM];
    __shared__ int s_hit[BM_MAXM], s_par[BM_MAXM], s_id[BM_MAXM], s_mf[MM355_BEAM_MAX + BM_MAXM], s_me[MM355_BEAM_MAX + BM_MAXM][3];
    __shared__ int s_tok[MM355_BEAM_MAX], s_parent[MM355_BEAM_MAX], s_taken[MM355_BEAM_MAX + BM_MAXM], s_step;
    const int live = a.live[0];
    __syncthreads();                                         // (every thread holds the old flag before thread 0 replaces it)
    if (!live) return;
    const int K = a.K, M = a.M;
    if (threadIdx.x == 0) s_step = -1;
    if (threadIdx.x == 0 && (a.scal[1] < 0 || a.scal[1] >= a.max_new_tokens)) {
        a.live[0] = 0;                                       // a step the logs and the table have no row for: the search ends unwritten
    } else if (threadIdx.x == 0) {
        const int n = a.scal[1];
        const bool last = n + 1 >= a.max_new_tokens;
        bool all_hit = true, full = true;
        for (int c = 0; c < M; ++c) {
            const int idx = min(max(a.cand_idx[c], 0), K * a.V - 1);      // (a promise; clamped, so parent and id stay inside their tables)
            const int id = idx % a.V;
            bool hit = last;
            for (int e = 0; e < a.n_eos; ++e) hit |= id == a.eos[e];
            s_val[c] = a.cand_val[c]; s_par[c] = idx / a.V; s_id[c] = id; s_hit[c] = hit;
            all_hit &= hit;
        }
        for (int k = 0; k < K; ++k) full &= a.fin_flag[k] != 0;
        const int unsat = a.scal[0];
        // 3. the running beams: the K best of val + hit * -1e9
        for (int c = 0; c < M; ++c) s_ms[c] = s_val[c] + (s_hit[c] ? 1.f : 0.f) * BM_NEG;
        for (int c = 0; c < K + M; ++c) s_taken[c] = 0;
        float run0 = 0.f;
        for (int k = 0; k < K; ++k) {
            int best = -1;
            for (int c = 0; c < M; ++c)
                if (!s_taken[c] && (best < 0 || cand_beats(s_ms[c], c, s_ms[best], best))) best = c;
            s_taken[best] = 1;
            a.running[k] = s_ms[best];
            if (k == 0) run0 = s_ms[best];
            s_tok[k] = s_id[best]; s_parent[k] = s_par[best];
            a.tok[k] = s_id[best]; a.parent[k] = s_par[best];
            a.tok_log[(int64_t)n * K + k] = s_id[best];
            a.parent_log[(int64_t)n * K + k] = s_par[best];
        }
        // 4. the finished pool: the K best of (old pool, val / (n + 1)^length_penalty + three penalties)
        const float pw = a.len_pow[n];
        for (int k = 0; k < K; ++k) {
            s_ms[k] = a.fin_score[k]; s_mf[k] = a.fin_flag[k];
            for (int j = 0; j < 3; ++j) s_me[k][j] = a.fin_end[3 * k + j];
        }
        for (int c = 0; c < M; ++c) {
            const bool fin = s_hit[c] && c < K;
            float f = s_val[c] / pw;
            f += (full && a.early_stopping == 1 ? 1.f : 0.f) * BM_NEG;
            f += (unsat ? 0.f : 1.f) * BM_NEG;
            f += (fin ? 0.f : 1.f) * BM_NEG;
            s_ms[K + c] = f; s_mf[K + c] = fin;
            s_me[K + c][0] = n; s_me[K + c][1] = s_par[c]; s_me[K + c][2] = s_id[c];
        }
        for (int c = 0; c < K + M; ++c) s_taken[c] = 0;
        bool all_fin = true, any_nan = false;
        float mn = INFINITY;
        int newflag[MM355_BEAM_MAX];
        for (int k = 0; k < K; ++k) {
            int best = -1;
            for (int c = 0; c < K + M; ++c)
                if (!s_taken[c] && (best < 0 || cand_beats(s_ms[c], c, s_ms[best], best))) best = c;
            s_taken[best] = 1;
            const float sc = s_ms[best];
            a.fin_score[k] = sc; a.fin_flag[k] = s_mf[best];
            for (int j = 0; j < 3; ++j) a.fin_end[3 * k + j] = s_me[best][j];
            newflag[k] = s_mf[best];
            all_fin &= s_mf[best] != 0;
            any_nan |= sc != sc;
            mn = fminf(mn, sc);
        }
        if (any_nan) mn = __builtin_nanf("");                  // (torch.min hands a NaN on)
        // 5. the heuristic: can the best running beam still beat the worst finished hypothesis?
        const int n1 = n + 1;
        const float hyp = a.len_pow[(a.fixed_len ? a.max_new_tokens : n1) - 1];
        const float bestrun = run0 / hyp;
        bool any = false;
        for (int k = 0; k < K; ++k) any |= bestrun > (newflag[k] ? mn : BM_NEG);
        const int unsat1 = unsat && any;
        a.scal[0] = unsat1; a.scal[1] = n1;
        // 6. go on?
        if (!(unsat1 && !(all_fin && a.early_stopping == 1) && !all_hit)) a.live[0] = 0;
        s_step = n;
    }
    __syncthreads();
    const int s = s_step;
    if (s < 0) return;
    if (a.own_block) {
        // own row t < s of slot i is where its parent had it; row s is the one slot i appends itself in the next decode step.  A column is
        // read whole before it is written, so the gather runs in place.
        for (int t = threadIdx.x; t < s; t += 256) {
            uint8_t col[MM355_BEAM_MAX];
#pragma unroll
            for (int k = 0; k < MM355_BEAM_MAX; ++k) col[k] = k < K ? a.own_block[k * a.ld_ob + t] : 0;
#pragma unroll
            for (int k = 0; k < MM355_BEAM_MAX; ++k) {
                if (k < K) {
                    uint8_t v = 0;
#pragma unroll
                    for (int j = 0; j < MM355_BEAM_MAX; ++j) v = s_parent[k] == j ? col[j] : v;
                    a.own_block[k * a.ld_ob + t] = v;
                }
            }
        }
        if ((int)threadIdx.x < K) a.own_block[threadIdx.x * a.ld_ob + s] = (uint8_t)threadIdx.x;
    }
    if (a.x_in) {
        for (int k = 0; k < K; ++k) {
            const uint16_t* src = a.embed + (int64_t)s_tok[k] * a.ld_embed;
            for (int c = threadIdx.x * 8; c < a.h; c += 256 * 8) *(u32x4*)(a.x_in + k * a.ld_x + c) = *(const u32x4*)(src + c);
        }
    }
}

bool select_ok(int64_t K, int64_t V, int64_t M) {
    return K >= 1 && K <= MM355_BEAM_MAX && V >= 1 && V <= INT_MAX - 4096 && K * V <= INT_MAX && M >= K && M <= 9 * K && M <= K * V;
}

}  // namespace

extern "C" int64_t mm355_beam_select_rows_ws_bytes(int64_t K, int64_t V, int64_t M) {
    if (!select_ok(K, V, M)) return 0;
    return K * M * 8;                                        // one fp32 value and one int32 index per (row, candidate)
}

extern "C" int mm355_beam_select_rows_f32(const float* x, int64_t K, int64_t V, const float* running, int64_t M, float* stats, float* cand_val,
                                          int32_t* cand_idx, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!x || !running || !stats || !cand_val || !cand_idx || !workspace || !select_ok(K, V, M) || (((uintptr_t)workspace) & 3)
        || workspace_bytes < mm355_beam_select_rows_ws_bytes(K, V, M))
        return MM355_EINVAL;
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + K * M);
    hipLaunchKernelGGL(beam_rows_kernel, dim3((unsigned)K), dim3(BM_NT), 0, (hipStream_t)stream, x, (int)V, running, (int)M, stats, pv, pi);
    hipLaunchKernelGGL(beam_merge_kernel, dim3(1), dim3(BM_NT), 0, (hipStream_t)stream, (const float*)pv, (const int*)pi, (int)K, (int)M,
                       (int)(M < V ? M : V), cand_val, cand_idx);
    return mm_launch_status();
}

extern "C" int mm355_beam_advance(const float* cand_val, const int32_t* cand_idx, int64_t K, int64_t M, int64_t V, float* running,
                                  float* fin_score, int32_t* fin_flag, int32_t* fin_end, int32_t* scal, int32_t* live, int32_t* tok,
                                  int32_t* parent, int32_t* tok_log, int32_t* parent_log, int64_t log_cap, uint8_t* own_block,
                                  int64_t ld_own_block, const mm355_bf16* embed, int64_t ld_embed, int64_t embed_rows, mm355_bf16* x_in,
                                  int64_t ld_x, int64_t h, const float* len_pow, int max_new_tokens, float length_penalty, int early_stopping,
                                  const int32_t* eos_ids, int n_eos, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!cand_val || !cand_idx || !running || !fin_score || !fin_flag || !fin_end || !scal || !live || !tok || !parent || !tok_log || !parent_log
        || !len_pow)
        return MM355_EINVAL;
    if (!select_ok(K, V, M) || max_new_tokens < 1 || log_cap < max_new_tokens || early_stopping < 0 || early_stopping > 2
        || !(length_penalty == length_penalty) || n_eos < 0 || n_eos > MM355_GREEDY_MAX_EOS || (n_eos && !eos_ids))
        return MM355_EINVAL;
    if (own_block && ld_own_block < max_new_tokens) return MM355_EINVAL;
    if ((x_in != nullptr) != (embed != nullptr)) return MM355_EINVAL;
    if (x_in && (V > embed_rows || h < 1 || h > INT_MAX || (h & 7) || (ld_embed & 7) || (ld_x & 7) || ld_embed < h || ld_x < h
                 || !mm_aligned16(embed) || !mm_aligned16(x_in)))
        return MM355_EINVAL;
    AdvanceArgs a;
    a.cand_val = cand_val; a.cand_idx = cand_idx; a.K = (int)K; a.M = (int)M; a.V = (int)V;
    a.running = running; a.fin_score = fin_score; a.fin_flag = fin_flag; a.fin_end = fin_end; a.scal = scal; a.live = live;
    a.tok = tok; a.parent = parent; a.tok_log = tok_log; a.parent_log = parent_log;
    a.own_block = own_block; a.ld_ob = ld_own_block;
    a.embed = (const uint16_t*)embed; a.ld_embed = ld_embed; a.x_in = (uint16_t*)x_in; a.ld_x = ld_x; a.h = (int)h;
    a.len_pow = len_pow; a.max_new_tokens = max_new_tokens; a.early_stopping = early_stopping;
    a.fixed_len = early_stopping == 2 && length_penalty > 0.f;
    a.n_eos = n_eos;
    for (int e = 0; e < MM355_GREEDY_MAX_EOS; ++e) a.eos[e] = e < n_eos ? eos_ids[e] : -1;      // (eos_ids is HOST memory)
    hipLaunchKernelGGL(beam_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return mm_launch_status();
}

// Logits processors and per-token log-probabilities in the device token loop (functional.GreedyLoopGraph(processors=...)): the kernel that
// edits the fp32 logits rows before the pick (HF's repetition penalty, min-new-tokens and suppress-tokens processors, in that order) and
// the kernel that, after the pick and before mm355_greedy_advance, marks the picked id in the sequence's bitmap of seen ids and logs its
// log-probability.  The host-side models are metamorph_amd.functional.logits_process_host and token_note_host.
#include "argrows.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int LGT_NT = 1024;

struct ProcessArgs {
    float* x; int C;
    float penalty;                                           // 1: the penalty step is off
    const uint32_t* seen; int64_t seen_words;
    const int* total_out; int min_new_tokens;                // 0: the eos step is off
    const int* suppress; int64_t n_suppress;
    int n_eos;
    int eos[MM355_GREEDY_MAX_EOS];
};

// one workgroup per row.  A thread owns whole words of the bitmap (few bits are set in a run: the row is read only where they are), and
// the two lists are written after a barrier: an id that is marked AND listed ends at -inf, as in HF's order.
__global__ __launch_bounds__(LGT_NT) void logits_process_kernel(const ProcessArgs a) {
    const int r = blockIdx.x;
    float* row = a.x + (int64_t)r * a.C;
    if (a.penalty != 1.f) {
        const uint32_t* bits = a.seen + (int64_t)r * a.seen_words;
        const int words = (a.C + 31) >> 5;
        for (int w = threadIdx.x; w < words; w += LGT_NT) {
            uint32_t m = bits[w];
            if (w == words - 1 && (a.C & 31)) m &= (1u << (a.C & 31)) - 1u;      // (bits at positions >= C are ignored)
            while (m) {
                const int i = (w << 5) + __ffs((int)m) - 1;
                m &= m - 1;
                const float v = row[i];
                row[i] = v < 0.f ? v * a.penalty : v / a.penalty;
            }
        }
        __syncthreads();
    }
    if (a.min_new_tokens > 0 && a.total_out[r] < a.min_new_tokens && (int)threadIdx.x < a.n_eos) {
        const int e = a.eos[threadIdx.x];
        if (e >= 0 && e < a.C) row[e] = -INFINITY;
    }
    for (int64_t s = threadIdx.x; s < a.n_suppress; s += LGT_NT) {
        const int e = a.suppress[s];
        if (e >= 0 && e < a.C) row[e] = -INFINITY;
    }
}

// one workgroup per row: every thread decides the (uniform) branch from the state mm355_greedy_advance will read after it
__global__ __launch_bounds__(LGT_NT) void token_note_kernel(const float* __restrict__ x, int C, const int* __restrict__ tok,
                                                            const int* __restrict__ in_image, const int* __restrict__ n_img,
                                                            const int* __restrict__ done, const int* __restrict__ n_tokens,
                                                            int num_image_tokens, int token_cap, uint32_t* __restrict__ seen, int64_t seen_words,
                                                            float* __restrict__ logp_log) {
    __shared__ float red[LGT_NT / 64];
    const int r = blockIdx.x;
    const int t = tok[r], nt = n_tokens[r];
    if (done[r] || (in_image[r] && n_img[r] < num_image_tokens) || nt < 0 || nt >= token_cap || t < 0 || t >= C) return;
    if (seen && threadIdx.x == 0) seen[(int64_t)r * seen_words + (t >> 5)] |= 1u << (t & 31);
    if (!logp_log) return;
    const float* row = x + (int64_t)r * C;
    // the maximum, a NaN anywhere making it NaN (fmaxf drops NaNs: they are counted beside it)
    float m = -INFINITY, nan = 0.f;
    row_for_cols<LGT_NT>(row, C, [&](float v, int) {
        m = fmaxf(m, v);
        if (v != v) nan = 1.f;
    });
    m = block_max<LGT_NT>(m, red);
    nan = block_max<LGT_NT>(nan, red);
    float* out = logp_log + (int64_t)r * token_cap + nt;
    if (nan != 0.f || !(fabsf(m) < INFINITY)) {                // NaN, +inf, or a row of -inf only
        if (threadIdx.x == 0) *out = __builtin_nanf("");
        return;
    }
    // the sum as a fixed tree: thread t adds the columns t, t + 1024, ... in that order, then the wave butterflies and the 16 waves in order
    float acc = 0.f;
    row_for_cols<LGT_NT>(row, C, [&](float v, int) { acc += __expf(v - m); });      // (v = -inf: 0)
    const float z = block_sum<LGT_NT>(acc, red);
    if (threadIdx.x == 0) *out = row[t] - m - logf(z);
}

bool rows_ok(int64_t R, int64_t C) { return R >= 1 && C >= 1 && C <= INT_MAX - 4096 && R <= 65535; }    // mm355_argmax_rows_f32's bounds

}  // namespace

extern "C" int mm355_logits_process_rows_f32(float* x, int64_t R, int64_t C, float penalty, const uint32_t* seen, int64_t seen_words,
                                             const int32_t* total_out, int min_new_tokens, const int32_t* eos_ids, int n_eos,
                                             const int32_t* suppress_ids, int64_t n_suppress, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!x || !rows_ok(R, C) || !(penalty > 0.f) || !(penalty < INFINITY)) return MM355_EINVAL;
    if (penalty != 1.f && (!seen || seen_words < (C + 31) / 32)) return MM355_EINVAL;
    if (min_new_tokens > 0 && !total_out) return MM355_EINVAL;
    if (n_eos < 0 || n_eos > MM355_GREEDY_MAX_EOS || (n_eos && !eos_ids) || n_suppress < 0 || (n_suppress && !suppress_ids)) return MM355_EINVAL;
    ProcessArgs a;
    a.x = x; a.C = (int)C; a.penalty = seen ? penalty : 1.f; a.seen = seen; a.seen_words = seen_words;
    a.total_out = total_out; a.min_new_tokens = min_new_tokens > 0 ? min_new_tokens : 0;
    a.suppress = suppress_ids; a.n_suppress = n_suppress; a.n_eos = n_eos;
    for (int e = 0; e < MM355_GREEDY_MAX_EOS; ++e) a.eos[e] = e < n_eos ? eos_ids[e] : -1;      // (eos_ids is HOST memory)
    if (a.penalty == 1.f && (!a.min_new_tokens || !n_eos) && !n_suppress) return MM355_OK;       // nothing to edit: no launch
    hipLaunchKernelGGL(logits_process_kernel, dim3((unsigned)R), dim3(LGT_NT), 0, (hipStream_t)stream, a);
    return mm_launch_status();
}

extern "C" int mm355_token_note_rows_f32(const float* x, int64_t R, int64_t C, const int32_t* tok, const int32_t* in_image, const int32_t* n_img,
                                         const int32_t* done, const int32_t* n_tokens, int num_image_tokens, int64_t token_cap, uint32_t* seen,
                                         int64_t seen_words, float* logp_log, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!x || !tok || !in_image || !n_img || !done || !n_tokens || !rows_ok(R, C) || token_cap < 0 || token_cap > INT_MAX) return MM355_EINVAL;
    if ((!seen && !logp_log) || (seen && seen_words < (C + 31) / 32)) return MM355_EINVAL;
    hipLaunchKernelGGL(token_note_kernel, dim3((unsigned)R), dim3(LGT_NT), 0, (hipStream_t)stream, x, (int)C, tok, in_image, n_img, done, n_tokens,
                       num_image_tokens, (int)token_cap, seen, seen_words, logp_log);
    return mm_launch_status();
}

// Prompt-lookup speculative decoding in the device token loop (functional.SpecGreedyLoopGraph): a step carries n = K + 1 rows per sequence
// -- its real next input and up to K guessed next tokens -- through the decoder, and these two kernels stand around it.
//   ngram_draft_kernel:  the guesses, looked up in the sequence's own text (HF's PromptLookupCandidateGenerator.get_candidates), and the
//                        step's input rows, positions and mode mask built from them (host model: functional.prompt_lookup_host).
//   spec_verify_kernel:  the reference loop's transition (greedy.hip: greedy_advance_kernel, functional.greedy_advance_host) run over
//                        the rows of one sequence for as long as the guesses hold (host model: functional.spec_advance_host).
// One workgroup per sequence in both; every branch is uniform over the workgroup (every thread reads the same words and keeps the state
// in registers), thread 0 writes the words back, all threads copy rows with 16-byte vectors.
#include "mm355_common.h"

#include <limits.h>

namespace {

constexpr int SPEC_NT = 256;

MM_DEV void copy_row(uint16_t* __restrict__ dst, const uint16_t* __restrict__ src, int h) {
    for (int c = threadIdx.x * 8; c < h; c += SPEC_NT * 8) *(u32x4*)(dst + c) = *(const u32x4*)(src + c);
}

MM_DEV void zero_row(uint16_t* __restrict__ dst, int h) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int c = threadIdx.x * 8; c < h; c += SPEC_NT * 8) *(u32x4*)(dst + c) = z;
}

struct DraftArgs {
    const int* hist; int64_t hist_cap; const int* hist_len;   // [B, hist_cap] the lookup ids followed by the logged ids; [B]
    const int *done, *in_image, *pos;                         // [B] each: the loop's state and the cache's write positions
    const uint16_t* embed; int64_t ld_embed;
    int *drafts, *n_draft;                                    // [B, K], [B]
    uint16_t* x_in; int64_t ld_x;                             // [B * (K + 1), h]
    int *pos_rows, *mask_rows;                                // [B * (K + 1)] each
    int K, N, C, h;
};

// The lowest index whose window equals the last m ids and whose continuation begins with an id of [0, C): every thread scans the indices
// tid, tid + 256, ... in rising order and stops at its first hit, then a minimum over the workgroup in fixed order (wave, then LDS).
__global__ __launch_bounds__(SPEC_NT) void ngram_draft_kernel(const DraftArgs g) {
    __shared__ int s_min[SPEC_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, n = g.K + 1;
    if (tid < n) g.pos_rows[b * n + tid] = g.pos[b] + tid;  // (also for a finished sequence: its rows keep landing above its length)
    if (g.done[b]) return;                                   // a finished sequence: nothing else is written (its drafts and input rows stay)
    const int* H = g.hist + (int64_t)b * g.hist_cap;
    const int cap = g.hist_cap < INT_MAX ? (int)g.hist_cap : INT_MAX;
    const int len = max(0, min(g.hist_len[b], cap));
    const int in_image = g.in_image[b];
    int start = -1;                                          // where the continuation begins
    if (!in_image) {
        for (int m = min(g.N, len - 1); m >= 1; --m) {
            int best = INT_MAX;
            for (int idx = tid; idx + m < len; idx += SPEC_NT) {     // (idx + m == len is the trailing occurrence: nothing follows it)
                const int c = H[idx + m];
                if (c < 0 || c >= g.C) continue;
                bool eq = true;
                for (int j = 0; j < m; ++j) eq &= H[idx + j] == H[len - m + j];
                if (eq) { best = idx; break; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
            if ((tid & 63) == 0) s_min[tid >> 6] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < SPEC_NT / 64; ++w) best = min(best, s_min[w]);
            __syncthreads();                                 // (s_min is written again for the next m)
            if (best != INT_MAX) { start = best + m; break; }
        }
    }
    int nd = 0;
    if (start >= 0)
        while (nd < g.K && start + nd < len && H[start + nd] >= 0 && H[start + nd] < g.C) ++nd;
    if (tid < g.K) g.drafts[b * g.K + tid] = tid < nd ? H[start + tid] : -1;
    if (tid == 0) g.n_draft[b] = nd;
    if (tid < n) g.mask_rows[b * n + tid] = tid == 0 ? in_image : 0;
    for (int j = 0; j < g.K; ++j) {
        uint16_t* dst = g.x_in + ((int64_t)b * n + 1 + j) * g.ld_x;
        if (j < nd) copy_row(dst, g.embed + (int64_t)H[start + j] * g.ld_embed, g.h);
        else zero_row(dst, g.h);
    }
}

struct VerifyArgs {
    const int* tok;                                          // [B * (K + 1)] the argmax of every row
    const int *drafts, *n_draft;                             // [B, K], [B]
    int *in_image, *n_img, *total_out, *done, *n_tokens, *n_z, *live;
    const uint16_t* embed; int64_t ld_embed; int embed_rows;
    const uint16_t* fed; int64_t ld_fed;                     // [B * (K + 1), h] the rows the lm_head saw
    const uint16_t* pred_z; int64_t ld_z;                    // [B * (K + 1), Dz]
    uint16_t* x_in; int64_t ld_x;
    int* tok_log; int token_cap;
    uint16_t* z_log; int z_cap;
    int* hist; int64_t hist_cap; int* hist_len;
    int *pos, *len;                                          // the cache's pos_dev / len_dev
    int* acc_log; int acc_cap; int* n_steps;
    int K, h, Dz, start_id, end_id, num_image_tokens, max_new_tokens, n_eos, count_step;
    int eos[MM355_GREEDY_MAX_EOS];
};

__global__ __launch_bounds__(SPEC_NT) void spec_verify_kernel(const VerifyArgs g) {
    const int b = blockIdx.x, n = g.K + 1;
    if (g.done[b]) return;
    int in_image = g.in_image[b], n_img = g.n_img[b], total_out = g.total_out[b], n_tokens = g.n_tokens[b], n_z = g.n_z[b];
    int hl = g.hist_len[b];
    const int nd = max(0, min(g.n_draft[b], g.K));
    __syncthreads();                                         // (every thread holds the old state before thread 0 replaces it)
    const uint16_t* next = nullptr;
    int a = 0, done = 0;
    for (int i = 0;; ++i) {                                  // one iteration of greedy_advance_kernel per trip, on row (b, i)
        const int r = b * n + i, tok = g.tok[r];
        const bool image_row = in_image && n_img < g.num_image_tokens;
        ++a;
        if (image_row ? n_z >= g.z_cap : (n_tokens >= g.token_cap || tok < 0 || tok >= g.embed_rows)) {
            done = 1;                                        // a full log, or an id that is no row of the embedding: done, nothing logged
            break;
        }
        if (image_row) {
            next = g.fed + r * g.ld_fed;
            copy_row(g.z_log + ((int64_t)b * g.z_cap + n_z) * g.Dz, g.pred_z + r * g.ld_z, g.Dz);
        } else {
            next = g.embed + (int64_t)tok * g.ld_embed;
        }
        if (!in_image && tok == g.start_id) {
            in_image = 1;
        } else if (image_row) {
            ++n_img;
            ++n_z;
            if (n_img == g.num_image_tokens) in_image = 0;
        } else if (tok == g.end_id) {
            in_image = 0;
            n_img = 0;
        }
        if (!image_row) {
            if (threadIdx.x == 0) {
                g.tok_log[(int64_t)b * g.token_cap + n_tokens] = tok;
                if (hl >= 0 && hl < g.hist_cap) g.hist[(int64_t)b * g.hist_cap + hl] = tok;
            }
            ++n_tokens;
            if (hl >= 0 && hl < g.hist_cap) ++hl;
        }
        ++total_out;
        bool stop = total_out > g.max_new_tokens;
        for (int e = 0; e < g.n_eos; ++e) stop |= tok == g.eos[e];
        if (stop) done = 1;
        // go on only while the next row's input was this id as a plain token row: not after an image row (the next input is the fed
        // row), not into image mode (the next row's head mask is 1), not past the drafts, not after a draft that missed
        if (done || image_row || in_image || i >= nd || tok != g.drafts[b * g.K + i]) break;
    }
    if (next) copy_row(g.x_in + (int64_t)b * n * g.ld_x, next, g.h);
    if (threadIdx.x != 0) return;
    g.in_image[b] = in_image; g.n_img[b] = n_img; g.total_out[b] = total_out; g.n_tokens[b] = n_tokens; g.n_z[b] = n_z;
    g.hist_len[b] = hl;
    if (g.count_step) {
        g.pos[b] += a;
        g.len[b] += a;
        const int s = g.n_steps[b];
        if (s >= 0 && s < g.acc_cap) { g.acc_log[(int64_t)b * g.acc_cap + s] = a; g.n_steps[b] = s + 1; }
    }
    if (done) { g.done[b] = 1; atomicSub(g.live, 1); }
}

bool rows_ok(const void* p, int64_t ld, int64_t w) { return p && mm_aligned16(p) && !(ld & 7) && ld >= w; }

}  // namespace

extern "C" int mm355_ngram_draft_rows(const int32_t* hist, int64_t hist_cap, const int32_t* hist_len, const int32_t* done, const int32_t* in_image,
                                      const int32_t* pos, int64_t B, int K, int N, int64_t C, const mm355_bf16* embed, int64_t ld_embed,
                                      int64_t embed_rows, int32_t* drafts, int32_t* n_draft, mm355_bf16* x_in, int64_t ld_x, int64_t h,
                                      int32_t* pos_rows, int32_t* mask_rows, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!hist || !hist_len || !done || !in_image || !pos || !drafts || !n_draft || !pos_rows || !mask_rows) return MM355_EINVAL;
    if (B < 1 || K < 1 || K > MM355_SPEC_MAX_DRAFT || N < 1 || N > MM355_SPEC_MAX_NGRAM || B * (K + 1) > INT_MAX || hist_cap < 1 || C < 1
        || C > embed_rows || embed_rows > INT_MAX || h < 1 || h > INT_MAX || (h & 7) || !rows_ok(embed, ld_embed, h) || !rows_ok(x_in, ld_x, h))
        return MM355_EINVAL;
    DraftArgs g;
    g.hist = hist; g.hist_cap = hist_cap; g.hist_len = hist_len; g.done = done; g.in_image = in_image; g.pos = pos;
    g.embed = (const uint16_t*)embed; g.ld_embed = ld_embed; g.drafts = drafts; g.n_draft = n_draft; g.x_in = (uint16_t*)x_in; g.ld_x = ld_x;
    g.pos_rows = pos_rows; g.mask_rows = mask_rows; g.K = K; g.N = N; g.C = (int)C; g.h = (int)h;
    hipLaunchKernelGGL(ngram_draft_kernel, dim3((unsigned)B), dim3(SPEC_NT), 0, (hipStream_t)stream, g);
    return mm_launch_status();
}

extern "C" int mm355_spec_verify_advance(const int32_t* tok, const int32_t* drafts, const int32_t* n_draft, int64_t B, int K, int64_t C,
                                         int32_t* in_image, int32_t* n_img, int32_t* total_out, int32_t* done, int32_t* n_tokens, int32_t* n_z,
                                         int32_t* live, const mm355_bf16* embed, int64_t ld_embed, int64_t embed_rows, const mm355_bf16* fed,
                                         int64_t ld_fed, const mm355_bf16* pred_z, int64_t ld_z, mm355_bf16* x_in, int64_t ld_x, int64_t h,
                                         int64_t Dz, int32_t* tok_log, int64_t token_cap, mm355_bf16* z_log, int64_t z_cap, int32_t* hist,
                                         int64_t hist_cap, int32_t* hist_len, int32_t* pos, int32_t* len, int32_t* acc_log, int64_t acc_cap,
                                         int32_t* n_steps, int count_step, int start_id, int end_id, int num_image_tokens, int max_new_tokens,
                                         const int32_t* eos_ids, int n_eos, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!tok || !drafts || !n_draft || !in_image || !n_img || !total_out || !done || !n_tokens || !n_z || !live || !tok_log || !z_log || !hist
        || !hist_len)
        return MM355_EINVAL;
    if (count_step && (!pos || !len || !acc_log || !n_steps)) return MM355_EINVAL;
    if (B < 1 || K < 1 || K > MM355_SPEC_MAX_DRAFT || B * (K + 1) > INT_MAX || C < 1 || C > embed_rows || embed_rows > INT_MAX || n_eos < 0
        || n_eos > MM355_GREEDY_MAX_EOS || (n_eos && !eos_ids) || hist_cap < 1)
        return MM355_EINVAL;
    if (h < 1 || Dz < 1 || h > INT_MAX || Dz > INT_MAX || (h & 7) || (Dz & 7) || !rows_ok(embed, ld_embed, h) || !rows_ok(fed, ld_fed, h)
        || !rows_ok(pred_z, ld_z, Dz) || !rows_ok(x_in, ld_x, h) || !mm_aligned16(z_log) || token_cap < 0 || z_cap < 0 || acc_cap < 0
        || token_cap > INT_MAX || z_cap > INT_MAX || acc_cap > INT_MAX)
        return MM355_EINVAL;
    VerifyArgs g;
    g.tok = tok; g.drafts = drafts; g.n_draft = n_draft;
    g.in_image = in_image; g.n_img = n_img; g.total_out = total_out; g.done = done; g.n_tokens = n_tokens; g.n_z = n_z; g.live = live;
    g.embed = (const uint16_t*)embed; g.ld_embed = ld_embed; g.embed_rows = (int)embed_rows;
    g.fed = (const uint16_t*)fed; g.ld_fed = ld_fed; g.pred_z = (const uint16_t*)pred_z; g.ld_z = ld_z;
    g.x_in = (uint16_t*)x_in; g.ld_x = ld_x; g.tok_log = tok_log; g.token_cap = (int)token_cap; g.z_log = (uint16_t*)z_log; g.z_cap = (int)z_cap;
    g.hist = hist; g.hist_cap = hist_cap; g.hist_len = hist_len; g.pos = pos; g.len = len; g.acc_log = acc_log; g.acc_cap = (int)acc_cap;
    g.n_steps = n_steps; g.K = K; g.h = (int)h; g.Dz = (int)Dz; g.start_id = start_id; g.end_id = end_id;
    g.num_image_tokens = num_image_tokens; g.max_new_tokens = max_new_tokens; g.n_eos = n_eos; g.count_step = count_step;
    for (int e = 0; e < MM355_GREEDY_MAX_EOS; ++e) g.eos[e] = e < n_eos ? eos_ids[e] : -1;      // (eos_ids is HOST memory)
    hipLaunchKernelGGL(spec_verify_kernel, dim3((unsigned)B), dim3(SPEC_NT), 0, (hipStream_t)stream, g);
    return mm_launch_status();
}

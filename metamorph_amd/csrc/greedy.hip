// The greedy loop's per-token tail on the device (reference metamorph_llama.py:502-597): argmax of the fp32 logits rows, the row select
// that picks the lm_head input per sequence, and the reference loop's mode state machine with the gather of the next input row.  With
// these three the host reads nothing per token: one captured graph is one whole token for every sequence (functional.GreedyLoopGraph).
#include "argrows.h"

#include <limits.h>

namespace {

constexpr int ARG_NT = 256;
constexpr int ARG_CHUNK = 4096;                              // columns per (row, chunk) partial: 16 per thread

// the workgroup's winner in thread 0 (blockDim.x = ARG_NT)
MM_DEV void arg_block(float& v, int& i, float* sv, int* si) {
    arg_wave(v, i);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (l == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < ARG_NT / 64; ++k)
            if (arg_beats(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; }
    }
}

// stage 1: workgroup (chunk, row) -> the winner of columns [chunk * ARG_CHUNK, +ARG_CHUNK) of that row
__global__ __launch_bounds__(ARG_NT) void argmax_partial_kernel(const float* __restrict__ x, int C, int chunks, float* __restrict__ pv,
                                                                int* __restrict__ pi) {
    __shared__ float sv[ARG_NT / 64];
    __shared__ int si[ARG_NT / 64];
    const int chunk = blockIdx.x, r = blockIdx.y;
    const float* row = x + (int64_t)r * C;
    const int c0 = chunk * ARG_CHUNK, c1 = min(c0 + ARG_CHUNK, C);
    float v = -INFINITY;
    int i = INT_MAX;                                        // (loses every tie, so a row of -inf yields its first column)
    for (int c = c0 + (int)threadIdx.x; c < c1; c += ARG_NT) {
        const float cv = row[c];
        if (arg_beats(cv, c, v, i)) { v = cv; i = c; }
    }
    arg_block(v, i, sv, si);
    if (threadIdx.x == 0) {
        pv[(int64_t)r * chunks + chunk] = v;
        pi[(int64_t)r * chunks + chunk] = i;
    }
}

// stage 2: one workgroup per row over its partials
__global__ __launch_bounds__(ARG_NT) void argmax_final_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int chunks,
                                                              int* __restrict__ out) {
    __shared__ float sv[ARG_NT / 64];
    __shared__ int si[ARG_NT / 64];
    const int r = blockIdx.x;
    float v = -INFINITY;
    int i = INT_MAX;
    for (int c = threadIdx.x; c < chunks; c += ARG_NT) {
        const float cv = pv[(int64_t)r * chunks + c];
        const int ci = pi[(int64_t)r * chunks + c];
        if (arg_beats(cv, ci, v, i)) { v = cv; i = ci; }
    }
    arg_block(v, i, sv, si);
    if (threadIdx.x == 0) out[r] = i;
}

__global__ __launch_bounds__(256) void rows_select_kernel(const uint16_t* __restrict__ a, int64_t lda, const uint16_t* __restrict__ b, int64_t ldb,
                                                          const int* __restrict__ mask, uint16_t* __restrict__ out, int64_t ldo, int h) {
    const int r = blockIdx.x;
    const uint16_t* src = mask[r] ? a + r * lda : b + r * ldb;
    for (int c = threadIdx.x * 8; c < h; c += 256 * 8)
        *(u32x4*)(out + r * ldo + c) = *(const u32x4*)(src + c);
}

struct GreedyArgs {
    const int* tok;                                          // [B] this step's argmax ids
    int *in_image, *n_img, *total_out, *done, *n_tokens, *n_z, *live;
    const uint16_t* embed; int64_t ld_embed; int embed_rows;
    const uint16_t* fed; int64_t ld_fed;                     // [B, h] the rows the lm_head saw
    const uint16_t* pred_z; int64_t ld_z;                    // [B, Dz]
    uint16_t* x_in; int64_t ld_x;
    int* tok_log; int token_cap;
    uint16_t* z_log; int z_cap;
    int h, Dz, start_id, end_id, num_image_tokens, max_new_tokens, n_eos;
    int eos[MM355_GREEDY_MAX_EOS];
};

// one workgroup per sequence: every thread decides the (uniform) branch from the state it read, thread 0 writes the state back, all copy rows
__global__ __launch_bounds__(256) void greedy_advance_kernel(const GreedyArgs g) {
    const int b = blockIdx.x;
    if (g.done[b]) return;
    const int tok = g.tok[b], in_image = g.in_image[b], n_img = g.n_img[b], total_out = g.total_out[b], n_tokens = g.n_tokens[b],
              n_z = g.n_z[b];
    __syncthreads();                                         // (every thread holds the old state before thread 0 replaces it)
    const bool image_row = in_image && n_img < g.num_image_tokens;
    // a log that is full, or an id that is no row of the embedding (cannot come out of mm355_argmax_rows_f32), ends the sequence unwritten
    const bool refuse = image_row ? n_z >= g.z_cap : (n_tokens >= g.token_cap || tok < 0 || tok >= g.embed_rows);
    if (refuse) {
        if (threadIdx.x == 0) { g.done[b] = 1; atomicSub(g.live, 1); }
        return;
    }
    const uint16_t* next;
    if (image_row) {
        next = g.fed + b * g.ld_fed;
        uint16_t* z = g.z_log + ((int64_t)b * g.z_cap + n_z) * g.Dz;
        for (int c = threadIdx.x * 8; c < g.Dz; c += 256 * 8) *(u32x4*)(z + c) = *(const u32x4*)(g.pred_z + b * g.ld_z + c);
    } else {
        next = g.embed + (int64_t)tok * g.ld_embed;
    }
    for (int c = threadIdx.x * 8; c < g.h; c += 256 * 8) *(u32x4*)(g.x_in + b * g.ld_x + c) = *(const u32x4*)(next + c);
    if (threadIdx.x != 0) return;
    if (!in_image && tok == g.start_id) {
        g.in_image[b] = 1;
    } else if (image_row) {
        g.n_img[b] = n_img + 1;
        g.n_z[b] = n_z + 1;
        if (n_img + 1 == g.num_image_tokens) g.in_image[b] = 0;
    } else if (tok == g.end_id) {
        g.in_image[b] = 0;
        g.n_img[b] = 0;
    }
    if (!image_row) {
        g.tok_log[(int64_t)b * g.token_cap + n_tokens] = tok;
        g.n_tokens[b] = n_tokens + 1;
    }
    g.total_out[b] = total_out + 1;
    bool stop = total_out + 1 > g.max_new_tokens;
    for (int e = 0; e < g.n_eos; ++e) stop |= tok == g.eos[e];
    if (stop) { g.done[b] = 1; atomicSub(g.live, 1); }
}

int argmax_chunks(int64_t C) { return (int)((C + ARG_CHUNK - 1) / ARG_CHUNK); }

}  // namespace

extern "C" int64_t mm355_argmax_rows_ws_bytes(int64_t R, int64_t C) {
    if (R < 1 || C < 1) return 0;
    return R * argmax_chunks(C) * 8;                         // one fp32 value and one int32 index per (row, chunk)
}

extern "C" int mm355_argmax_rows_f32(const float* x, int64_t R, int64_t C, int32_t* out, void* workspace, int64_t workspace_bytes, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!x || !out || !workspace || R < 1 || C < 1 || C > INT_MAX - ARG_CHUNK || R > 65535 || (((uintptr_t)workspace) & 3)
        || workspace_bytes < mm355_argmax_rows_ws_bytes(R, C))
        return MM355_EINVAL;
    const int chunks = argmax_chunks(C);
    float* pv = (float*)workspace;
    int* pi = (int*)(pv + R * chunks);
    hipLaunchKernelGGL(argmax_partial_kernel, dim3(chunks, (unsigned)R), dim3(ARG_NT), 0, (hipStream_t)stream, x, (int)C, chunks, pv, pi);
    hipLaunchKernelGGL(argmax_final_kernel, dim3((unsigned)R), dim3(ARG_NT), 0, (hipStream_t)stream, (const float*)pv, (const int*)pi, chunks, out);
    return mm_launch_status();
}

extern "C" int mm355_rows_select_bf16(const mm355_bf16* a, int64_t lda, const mm355_bf16* b, int64_t ldb, const int32_t* mask, mm355_bf16* out,
                                      int64_t ldo, int64_t R, int64_t h, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!a || !b || !mask || !out || R < 1 || h < 1 || h > INT_MAX || (h & 7) || (lda & 7) || (ldb & 7) || (ldo & 7) || lda < h || ldb < h || ldo < h
        || !mm_aligned16(a) || !mm_aligned16(b) || !mm_aligned16(out))
        return MM355_EINVAL;
    hipLaunchKernelGGL(rows_select_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)a, lda, (const uint16_t*)b, ldb,
                       mask, (uint16_t*)out, ldo, (int)h);
    return mm_launch_status();
}

extern "C" int mm355_greedy_advance(const int32_t* tok, int64_t B, int64_t C, int32_t* in_image, int32_t* n_img, int32_t* total_out, int32_t* done,
                                    int32_t* n_tokens, int32_t* n_z, int32_t* live, const mm355_bf16* embed, int64_t ld_embed,
                                    int64_t embed_rows, const mm355_bf16* fed, int64_t ld_fed, const mm355_bf16* pred_z, int64_t ld_z,
                                    mm355_bf16* x_in, int64_t ld_x, int64_t h, int64_t Dz, int32_t* tok_log, int64_t token_cap,
                                    mm355_bf16* z_log, int64_t z_cap, int start_id, int end_id, int num_image_tokens, int max_new_tokens,
                                    const int32_t* eos_ids, int n_eos, void* stream) {
    (void)hipGetLastError();   // drop any stale, unrelated runtime status before we launch
    if (!tok || !in_image || !n_img || !total_out || !done || !n_tokens || !n_z || !live || !embed || !fed || !pred_z || !x_in || !tok_log || !z_log)
        return MM355_EINVAL;
    if (B < 1 || B > INT_MAX || C < 1 || C > embed_rows || embed_rows > INT_MAX || n_eos < 0 || n_eos > MM355_GREEDY_MAX_EOS || (n_eos && !eos_ids))
        return MM355_EINVAL;
    if (h < 1 || Dz < 1 || h > INT_MAX || Dz > INT_MAX || (h & 7) || (Dz & 7) || (ld_embed & 7) || (ld_fed & 7) || (ld_z & 7) || (ld_x & 7)
        || ld_embed < h || ld_fed < h || ld_x < h || ld_z < Dz || token_cap < 0 || z_cap < 0 || token_cap > INT_MAX || z_cap > INT_MAX
        || !mm_aligned16(embed) || !mm_aligned16(fed) || !mm_aligned16(pred_z) || !mm_aligned16(x_in) || !mm_aligned16(z_log))
        return MM355_EINVAL;
    GreedyArgs g;
    g.tok = tok; g.in_image = in_image; g.n_img = n_img; g.total_out = total_out; g.done = done; g.n_tokens = n_tokens; g.n_z = n_z; g.live = live;
    g.embed = (const uint16_t*)embed; g.ld_embed = ld_embed; g.embed_rows = (int)embed_rows;
    g.fed = (const uint16_t*)fed; g.ld_fed = ld_fed; g.pred_z = (const uint16_t*)pred_z; g.ld_z = ld_z;
    g.x_in = (uint16_t*)x_in; g.ld_x = ld_x; g.tok_log = tok_log; g.token_cap = (int)token_cap; g.z_log = (uint16_t*)z_log; g.z_cap = (int)z_cap;
    g.h = (int)h; g.Dz = (int)Dz; g.start_id = start_id; g.end_id = end_id; g.num_image_tokens = num_image_tokens;
    g.max_new_tokens = max_new_tokens; g.n_eos = n_eos;
    for (int e = 0; e < MM355_GREEDY_MAX_EOS; ++e) g.eos[e] = e < n_eos ? eos_ids[e] : -1;      // (eos_ids is HOST memory)
    hipLaunchKernelGGL(greedy_advance_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, g);
    return mm_launch_status();
}

// What the kernels over rows of fp32 logits share: the order of torch.argmax on (value, index) pairs (the argmax of the greedy loop in
// greedy.hip and the sampler's fall-back to it in sample.hip) and the walk of one workgroup over a row (sample.hip, logits.hip).
#pragma once
#include "mm355_common.h"

// torch.argmax's order: a NaN beats every number, among equals (and among NaNs) the lowest index wins.  A total order on (value, index)
// pairs with distinct indices, so any reduction tree gives the same winner.
MM_DEV bool arg_beats(float cv, int ci, float bv, int bi) {
    const bool cn = cv != cv, bn = bv != bv;
    if (cn || bn) return cn && (!bn || ci < bi);
    return cv > bv || (cv == bv && ci < bi);
}

MM_DEV void arg_wave(float& v, int& i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(i, o, 64);
        if (arg_beats(ov, oi, v, i)) { v = ov; i = oi; }
    }
}

// f(value, column) over the columns tid, tid + NT, ... of a row in that order (blockDim.x = NT), 16 loads in flight per thread: one
// workgroup reads the row out of L2, and with one load per trip a pass is C / NT dependent L2 latencies long
template <int NT, class Fn>
MM_DEV void row_for_cols(const float* __restrict__ row, int C, Fn f) {
    constexpr int U = 16;
    int c = threadIdx.x;
    for (; (int64_t)c + (U - 1) * NT < C; c += U * NT) {
        float v[U];
#pragma unroll
        for (int j = 0; j < U; ++j) v[j] = row[c + j * NT];
#pragma unroll
        for (int j = 0; j < U; ++j) f(v[j], c + j * NT);
    }
    for (; c < C; c += NT) f(row[c], c);
}

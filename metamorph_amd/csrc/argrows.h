// The order of torch.argmax on (value, index) pairs, shared by the argmax of the greedy loop (greedy.hip) and the sampler's fall-back to it
// (sample.hip).
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

// rank_key.h — the order-preserving integer image of a score that the ranking kernels compare (ranking.hip, topk.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace dir {

// Ascending with the score for every non-NaN float; -0 and +0 share a key (they compare equal).  The smallest image is
// that of -inf, 0x007fffff: the values below it are free for what has to sort behind every number.
__device__ __forceinline__ uint32_t score_key_u32(float s) {
    if (s == 0.f) s = 0.f;                               // -0 -> +0
    const uint32_t b = __builtin_bit_cast(uint32_t, s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace dir

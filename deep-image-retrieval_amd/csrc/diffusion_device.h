// diffusion_device.h — what diffusion.hip (the solve over all N rows) and diffusion_local.hip (the solve of a query's top-T
// subgraph) share: the cut of a dot product into slabs and chains, and the power rule of the weights.
#pragma once
#include "dir_common.h"

// products THEN sums, never a fused multiply-add (see expand_lists.hip)
#pragma clang fp contract(off)

namespace dir {

constexpr int kDiffSlab = 256;     // rows per slab of a dot product
constexpr int kDiffChains = 64;    // chains of a slab: row r belongs to chain r mod 64
constexpr int kDiffPer = kDiffSlab / kDiffChains;   // rows of a chain

// w = v^gamma: gamma multiplications from 1 for an integer gamma in 0..64, powf otherwise (expand_lists.hip's rule)
__device__ __forceinline__ float diff_weight(float v, float gamma, int igamma) {
    if (igamma < 0) return powf(v, gamma);
    float w = 1.f;
    for (int e = 0; e < igamma; ++e) w = w * v;
    return w;
}

static inline int diff_igamma(float gamma) {
    const int ig = (int)gamma;
    return ((float)ig == gamma && ig >= 0 && ig <= 64) ? ig : -1;
}

}  // namespace dir

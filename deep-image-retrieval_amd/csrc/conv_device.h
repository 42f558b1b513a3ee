// conv_device.h — device-side plumbing every conv kernel shares: the LDS-DMA wrapper and its out-of-bounds offset, the
// buffer descriptor, the exact division by a launcher-prepared constant (host half: conv_igemm.h fastdiv_init), the
// wave-private LDS hand-off and the tail of the epilogue (residual add, ReLU, pack).  Each conv_*.hip keeps only what is its own.
#pragma once
#include "dir_common.h"

namespace dir {

// voffset beyond any descriptor (tensors are < 2^31 bytes): the DMA writes zeros.  2^31 cannot wrap
// in 32 bits when the scalar K offset is added, whichever way the bounds check treats soffset.
static constexpr uint32_t kOOB = 0x80000000u;

// Raw buffer descriptor over `bytes` of `ptr` (word 3 = 0x00020000: 32-bit raw access, out-of-range lanes read zeros).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* ptr, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, bytes, 0x00020000);
}

// 16 bytes per lane, global/L2 -> LDS at (wave-uniform `lds`) + lane * 16; `soff` rides in an SGPR.
// (Kept in a __device__ function: used directly inside the kernel template's lambda, hipcc 7.2
// silently drops the kernel's host stub.)
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, char* lds, uint32_t voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (DIR_LDS void*)lds, 16, voff, soff, 0, 0);
}

// n / d for n < 2^31 with (mul, shr) from fastdiv_init(d) (conv_igemm.h)
__device__ __forceinline__ uint32_t fast_div(uint32_t n, uint32_t mul, uint32_t shr) {
    return mul ? (__umulhi(n, mul) >> shr) : n;  // mul == 0 encodes division by 1
}

// What one lane of a wave wrote to LDS becomes visible to the other lanes of the SAME wave (wave-private staging passes:
// no workgroup barrier involved).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the tail of an epilogue: eight fp32 values of one pixel (+ residual) (ReLU) -> four packed words ---------------
template <class DT>
__device__ __forceinline__ void add_res8(float (&v)[8], u32x4_t rv) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float lo, hi;
        DT::unpack(rv[e], lo, hi);
        v[2 * e] += lo;
        v[2 * e + 1] += hi;
    }
}
__device__ __forceinline__ void relu8(float (&v)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = fmaxf(v[e], 0.f);
}
template <class DT>
__device__ __forceinline__ u32x4_t pack8(const float (&v)[8]) {
    u32x4_t ov;
#pragma unroll
    for (int e = 0; e < 4; ++e) ov[e] = DT::pack(v[2 * e], v[2 * e + 1]);
    return ov;
}

}  // namespace dir

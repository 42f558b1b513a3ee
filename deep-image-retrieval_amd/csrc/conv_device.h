// conv_device.h — device-side plumbing every conv kernel shares: the LDS-DMA wrapper and its out-of-bounds offset, the
// buffer descriptor, the exact division by a launcher-prepared constant (host half: conv_igemm.h fastdiv_init), the
// wave-private LDS hand-off, the implicit-GEMM lane geometry and K order, the bias-initialised accumulators and both epilogues:
// the staged one (epilogue_strip: through LDS, the kernel's callable owns address, mask, residual and store) with its tail
// (residual add, ReLU, pack), and the register one (swap_pack16).  Each conv_*.hip keeps only what is its own.
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

// 16 bytes per lane through a buffer descriptor, `soff` in an SGPR; a voffset beyond the descriptor (kOOB) drops the store.
// (In a __device__ function for dma16's reason: the epilogue callables are lambdas.)
__device__ __forceinline__ void bstore16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, int soff, u32x4_t v) {
    __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voff, soff, 0);
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

// ---- implicit GEMM: what one lane reads for LDS row (output pixel) m ------------------------------------------------------
// xbase: byte offset of tap (0, 0) of pixel m at 16-byte chunk `chunk` of the channel slice (may be negative); xmask: a
// bit per filter tap (R, S <= 4), set where the tap lies inside the image and m < a.M, in closed form: rows r in
// [max(0, -ih0), min(R, H - ih0)), columns s in [max(0, -iw0), min(S, W - iw0)).  CIN16 (the space-to-depth stem: one
// K-step per filter row, the lane's chunk is pixel chunk >> 1 of that row): a bit per filter ROW.
template <bool CIN16 = false, class A>
__device__ __forceinline__ void im2col_lane(const A& a, int m, int chunk, int& xbase, uint32_t& xmask) {
    const bool mvalid = m < a.M;
    const uint32_t mm = mvalid ? (uint32_t)m : 0u;
    const uint32_t b = fast_div(mm, a.div_ohw_mul, a.div_ohw_shr);
    const uint32_t rem = mm - b * (uint32_t)(a.OH * a.OW);
    const uint32_t oh = fast_div(rem, a.div_ow_mul, a.div_ow_shr);
    const uint32_t ow = rem - oh * (uint32_t)a.OW;
    const int ih0 = (int)oh * a.stride - a.pad;
    const int iw0 = (int)ow * a.stride - a.pad;
    xbase = (((int)b * a.H + ih0) * a.W + iw0) * a.Cin * 2 + chunk * 16;
    auto range_bits = [](int lo, int hi) -> uint32_t { return hi > lo ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u; };
    const uint32_t rbits = range_bits(max(0, -ih0), min(CIN16 ? 4 : a.R, a.H - ih0));
    if (CIN16) {
        const bool wok = (unsigned)(iw0 + (chunk >> 1)) < (unsigned)a.W;
        xmask = (mvalid && wok) ? rbits : 0u;
    } else {
        const uint32_t cbits = range_bits(max(0, -iw0), min(a.S, a.W - iw0));
        uint32_t mask = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) mask |= ((rbits >> r) & 1u) ? (cbits << (r * a.S)) : 0u;
        xmask = mvalid ? mask : 0u;
    }
}

// The K order of the implicit-GEMM kernels, one step per BK input channels of one filter tap: channel slice outermost,
// filter taps innermost (consecutive steps of a 3x3 conv read the SAME slice at pixel-shifted positions: L2 hits).  CIN16
// has one step per filter row and keeps row order.  Holds the step being ISSUED.
template <int BK, bool CIN16 = false>
struct KWalker {
    int tap = 0, cc = 0, r = 0, s = 0;
    template <class A>
    __device__ __forceinline__ void seek(const A& a, int t) {   // (split-K: start in the middle of the sequence)
        if (CIN16) {
            r = tap = t;
        } else {
            const int taps = a.R * a.S;
            cc = t / taps;
            tap = t - cc * taps;
            r = tap / a.S;
            s = tap - r * a.S;
        }
    }
    // bytes into the input, relative to tap (0, 0), with the channel slice `c` (default: this step's)
    template <class A>
    __device__ __forceinline__ int koff(const A& a, int c) const {
        return CIN16 ? (r * a.W * 32) : (((r * a.W + s) * a.Cin + c * BK) * 2);
    }
    template <class A>
    __device__ __forceinline__ int koff(const A& a) const { return koff(a, cc); }
    // index of this step's slice in a weight row; cpb = K-steps per filter tap
    __device__ __forceinline__ int wstep(int cpb) const { return CIN16 ? r : (tap * cpb + cc); }
    template <class A>
    __device__ __forceinline__ void advance(const A& a) {
        if (CIN16) {
            ++r;
            ++tap;
        } else {
            ++tap;
            if (++s == a.S) {
                s = 0;
                if (++r == a.R) {
                    r = 0;
                    tap = 0;
                    ++cc;
                }
            }
        }
    }
};

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

// ---- accumulators: after a 32x32 MFMA with swapped roles, acc[4 g + e] of a 32-channel block is channel 8 g + 4 lhi + e of
// pixel lrow.  They start at the folded-BN bias (or at zero: split-K partials, kernels that add the bias late). -------------
// acc[i][j] (i: channel blocks, j: pixel tiles) from b4(i, g), the four values of channels 8 g + 4 lhi .. + 3 of block i
template <int TN, int TM, class B4>
__device__ __forceinline__ void acc_init(f32x16_t (&acc)[TN][TM], B4&& b4) {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4_t v = b4(i, g);
#pragma unroll
            for (int j = 0; j < TM; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][4 * g + e] = v[e];
        }
}
// the four bias values of group g of the 32-channel block at `bias32` (LDS: a copy of the bias in shared memory)
template <bool LDS = false>
__device__ __forceinline__ f32x4_t bias4(const float* bias32, int g, int lhi) {
    if constexpr (LDS)
        return *(const f32x4_t*)(bias32 + 8 * g + 4 * lhi);
    else
        return *(const DIR_GLOBAL f32x4_t*)(bias32 + 8 * g + 4 * lhi);
}
// ... from `bias`, the bias of the wave's first channel
template <bool LDS = false, int TN, int TM>
__device__ __forceinline__ void acc_init_bias(f32x16_t (&acc)[TN][TM], const float* bias, int lhi) {
    acc_init(acc, [&](int i, int g) { return bias4<LDS>(bias + i * 32, g, lhi); });
}
template <int N>
__device__ __forceinline__ void acc_init_zero(f32x16_t (&acc)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[n][e] = 0.f;
}
template <int TN, int TM>
__device__ __forceinline__ void acc_init_zero(f32x16_t (&acc)[TN][TM]) {
#pragma unroll
    for (int i = 0; i < TN; ++i) acc_init_zero(acc[i]);
}
// ... 1-D tiles: TN channel blocks of ONE pixel tile,
template <bool LDS = false, int TN>
__device__ __forceinline__ void acc_init_bias_n(f32x16_t (&acc)[TN], const float* bias, int lhi) {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4_t v = bias4<LDS>(bias + i * 32, g, lhi);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[i][4 * g + e] = v[e];
        }
}
// TM pixel tiles of ONE channel block
template <bool LDS = false, int TM>
__device__ __forceinline__ void acc_init_bias_m(f32x16_t (&acc)[TM], const float* bias, int lhi) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4_t v = bias4<LDS>(bias, g, lhi);
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][4 * g + e] = v[e];
    }
}

// ---- the staged epilogue: a wave turns one 32-pixel strip of TN channel blocks into whole 16-byte runs through its own
// staging rows (fp32, pixel-major).  Lane (ecol, erow) = ((lane % LPR) * 8, lane / LPR) then owns 8 consecutive channels
// (ecol ..) of pixel pass * RPP + erow of the strip in each of NPASS passes. ----------------------------------------------
template <int TN>
struct Staged {
    static constexpr int EROW = TN * 128 + 16;   // bytes of one staging row: TN * 32 fp32 + pad; a wave owns 32 rows
    static constexpr int LPR = TN * 4;           // lanes covering one pixel row (8 channels each)
    static constexpr int RPP = 64 / LPR;         // pixel rows per pass
    static constexpr int NPASS = 32 / RPP;       // passes per strip
};
// blk(i) is the strip's i-th accumulator block; f(pass, mrow, v) gets the eight floats of pixel mrow and owns what differs
// between kernels: address and mask, residual, ReLU, pack, store.  Ends synchronised: the rows may be written again.
template <int TN, class BLK, class F>
__device__ __forceinline__ void epilogue_strip(char* ebase, int lrow, int lhi, int ecol, int erow, BLK&& blk, F&& f) {
    typedef Staged<TN> G;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x16_t& c = blk(i);
            const f32x4_t v = {c[4 * g + 0], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
            *(f32x4_t*)(ebase + lrow * G::EROW + (i * 32 + 8 * g + 4 * lhi) * 4) = v;
        }
    wave_lds_sync();
#pragma unroll
    for (int pass = 0; pass < G::NPASS; ++pass) {
        const int mrow = pass * G::RPP + erow;
        const f32x4_t f0 = *(const f32x4_t*)(ebase + mrow * G::EROW + ecol * 4);
        const f32x4_t f1 = *(const f32x4_t*)(ebase + mrow * G::EROW + ecol * 4 + 16);
        float v[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
        f(pass, mrow, v);
    }
    wave_lds_sync();
}

// ---- the register epilogue: channels h * 16 + lhi * 8 .. + 7 of pixel lrow, straight from one accumulator block.
// Group g of a block holds channels 8 g + 4 lhi .. + 3, i.e. each half-wave has one 8-byte half of the 16-byte runs 8 g .. 8 g + 7.
// (+ addend) (ReLU), pack, then v_permlane32_swap on the group pair (2 h, 2 h + 1) leaves lanes 0-31 with channels
// 16 h .. 16 h + 7 and lanes 32-63 with the next eight: one 16-byte store per lane.  `add`: four vectors, one per group, added
// to the accumulator first (a bias applied late, a residual).
template <class DT, class ADD>
__device__ __forceinline__ u32x4_t swap_pack16_(const f32x16_t& acc, int h, bool relu, ADD&& add) {
    uint32_t q2[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float x = add(acc[4 * (2 * h + q) + e], 2 * h + q, e);
            v[e] = relu ? fmaxf(x, 0.f) : x;
        }
        q2[q][0] = DT::pack(v[0], v[1]);
        q2[q][1] = DT::pack(v[2], v[3]);
    }
    const auto r0 = __builtin_amdgcn_permlane32_swap(q2[0][0], q2[1][0], false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(q2[0][1], q2[1][1], false, false);
    return u32x4_t{r0[0], r1[0], r0[1], r1[1]};
}
template <class DT>
__device__ __forceinline__ u32x4_t swap_pack16(const f32x16_t& acc, int h, bool relu) {
    return swap_pack16_<DT>(acc, h, relu, [](float x, int, int) { return x; });
}
template <class DT>
__device__ __forceinline__ u32x4_t swap_pack16(const f32x16_t& acc, int h, bool relu, const f32x4_t (&add)[4]) {
    return swap_pack16_<DT>(acc, h, relu, [&](float x, int g, int e) { return x + add[g][e]; });
}

}  // namespace dir

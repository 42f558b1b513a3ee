// index_fp4.hip — the fp4 descriptor index: 4-bit block-scaled codes, scanned on the scaled matrix cores.
//
// index_i8.hip's scan is a bytes kernel (2.06 GB of codes for 0.28 GB of scores at 70 x 1 006 322 x 2048).  A row of
// e2m1 codes with one e8m0 byte per block of 32 values and one fp32 power of two per row (include/dir_engine.h gives the
// definition) is half of those bytes, and v_mfma_scale_f32_32x32x64_f8f6f4 multiplies it as it lies.  The block
// exponents of a row are held within three binades, so every product of two dequantised values is a multiple of 1/64 of
// at most 36 and a sum of up to 7281 of them is exact in fp32 in any order: a score
//     scores[q][n] = (acc * qscales[q]) * bscales[n]
// is one defined fp32 number whatever the tiling, the K order, the rotation or the chunking, as in the int8 index.
//
// sim_fp4_kernel runs strip_stream.h's pipeline as sim_i8_kernel does - one 768-thread workgroup per 256 database rows,
// eight consumer waves of 32 rows against a block of 96 query rows (three f32x16 accumulators), three stages - with 256 k
// in a 128-byte stage row: a slab is 256 k, four 32x32x64 steps per accumulator block.  A lane's operand of a step is one
// 16-byte chunk = one block of 32 k, the same chunk of the row on both sides, and its scale byte is that block's.
//   Block bytes, query side: they ride in the image (768 bytes after the 12 KB of codes, already picked per lane half:
//     dword (lhi, row) = the bytes of blocks 2 s + lhi, s = 0 .. 3, so op_sel = s selects the step's byte).
//   Block bytes, database side: the consumer reads its row's 8 bytes of a slab from global memory with one 8-byte load, one
//     slab ahead.  Through the stage they would be 2 KB per slab in 8-byte pieces of rows [N][lde]: 256 lanes of DMA
//     issue for 1/16 of the bytes, against one load per lane that has a whole slab of MFMAs to hide behind.
// Rows are padded to 64 k (32 bytes) and not to a slab, so the last slab may hold 2, 4 or 6 of its 8 chunks: ChunkCutLoader
// cuts by chunk where StripLoader cuts by half (the codes pitch need not cover a whole slab); the block bytes' pitch does
// cover whole slabs (8 * ceil(D / 256)), the bytes of the blocks past D rounded up to 64 are replaced by 127 in the kernel.
#include "dir_common.h"
#include "flat_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the definition is in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kFp4MaxDim = 7281;            // 36 * 64 * 7281 = 16 775 424 < 2^24: every partial sum is exact in fp32
static constexpr int kFp4SlabCodes = kQB * kStripRow;             // 12288
static constexpr int kFp4SlabQ = kFp4SlabCodes + kStripPiece;     // + the block bytes (768 of a 1 KiB piece)
static constexpr int kFp4Stage = kStripSlab + kFp4SlabQ;
static constexpr int kFp4Stages = 3;
static constexpr int kFp4Lds = kFp4Stages * kFp4Stage;            // 138240 of 163840

int index_fp4_max_dim() { return kFp4MaxDim; }

// ---- quantisation ------------------------------------------------------------------------------------------------------
// One wave per row, quantize_rows_i8_kernel's walk: a lane owns quads of consecutive k, quad (c * 8 + i) * 64 + lane, so
// step (c, i) of the wave is slab c * 8 + i and eight neighbouring lanes hold one block of 32.  A row of up to 2048 values
// stays in registers between the pass that finds the row's top exponent and the pass that codes it.
__device__ __forceinline__ uint32_t fp4_code(float x, float inv) {
    const float y = __fmul_rn(__builtin_fabsf(x), inv);               // exact: inv is a power of two
    // nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, a midpoint to the even code, saturating
    const uint32_t c = (uint32_t)(y > 0.25f) + (uint32_t)(y >= 0.75f) + (uint32_t)(y > 1.25f) + (uint32_t)(y >= 1.75f) +
                       (uint32_t)(y > 2.5f) + (uint32_t)(y >= 3.5f) + (uint32_t)(y > 5.f);
    return c ? c | ((__builtin_bit_cast(uint32_t, x) >> 28) & 8u) : 0u;   // a value that rounds to zero is +0
}

__global__ void __launch_bounds__(256) quantize_rows_fp4_kernel(const float* __restrict__ X, int ldx, int N, int D,
                                                              uint8_t* __restrict__ codes, int ldc,
                                                              uint8_t* __restrict__ exps, int lde,
                                                              float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* row = X + (size_t)n * ldx;
    const bool vec = (ldx & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    const int Dp = pad64(D), T = fp4_slabs(D);
    const int chunks = (D + 2047) >> 11;
    f32x4_t v[8];
    uint32_t top = 0;                                   // the largest |x| as bits: an integer order on non-negative floats
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = load4_guarded(row, ((c * 8 + i) * 64 + lane) * 4, D, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = v[i][e];
                top = max(top, __builtin_bit_cast(uint32_t, xe) & 0x7fffffffu);
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d));
    const bool bad = top >= 0x7f800000u;                // an infinity or a NaN
    const int F = (int)(top >> 23);                     // the exponent field of amax; E = F - 129
    const bool zero = bad || F < 127 - 60;              // amax < 2^-60
    uint8_t* crow = codes + (size_t)n * ldc;
    uint8_t* erow = exps + (size_t)n * lde;
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (c * 8 + i >= T) continue;               // (wave-uniform: the shuffles below see all lanes)
            const int k = ((c * 8 + i) * 64 + lane) * 4;
            if (chunks > 1) v[i] = load4_guarded(row, k, D, vec);
            uint32_t bmax = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = v[i][e];
                bmax = max(bmax, __builtin_bit_cast(uint32_t, xe) & 0x7fffffffu);
            }
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) bmax = max(bmax, (uint32_t)__shfl_xor((int)bmax, d));
            const int m = max((int)(bmax >> 23), F - 2);                  // e_b clamped to [E - 2, E], as a field: e_b = m - 129
            const float inv = __builtin_bit_cast(float, (uint32_t)(256 - m) << 23);   // 2^-e_b
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= ((zero || k + e >= D) ? 0u : fp4_code(v[i][e], inv)) << (4 * e);
            if (k < Dp) *(uint16_t*)(crow + (k >> 1)) = (uint16_t)w;       // (k % 4 == 0, ldc % 2 == 0, codes 2-byte aligned)
            if ((lane & 7) == 0) erow[k >> 5] = (uint8_t)((zero || k >= D) ? 127 : 127 + m - F);
        }
    }
    if (lane == 0) scales[n] = bad ? __builtin_nanf("") : zero ? 0.f : __builtin_bit_cast(float, (uint32_t)(F - 2) << 23);
}

int quantize_rows_fp4(const float* X, int ldx, int N, int D, uint8_t* codes, int ldc, uint8_t* exps, int lde, float* scales,
                      hipStream_t stream) {
    return rows_launch("quantize_rows_fp4", "N", N, [&](unsigned blocks) {
        hipLaunchKernelGGL(quantize_rows_fp4_kernel, dim3(blocks), dim3(256), 0, stream, X, ldx, N, D, codes, ldc, exps, lde, scales);
    });
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// Query codes as an image of the LDS stages: [query block][K slab of 256][96 rows][128 bytes] with the database rows'
// swizzle, then [2 lane halves][96 rows] dwords of block bytes (see the head of the file) and zeros up to the piece.  Rows
// past Q and k past D are zero codes under the byte 127, so whatever the database codes hold beyond D multiply a zero.
__global__ void __launch_bounds__(256) fp4_image_kernel(const uint8_t* __restrict__ qcodes, int ldq,
                                                      const uint8_t* __restrict__ qexps, int ldqe, int Q, int D,
                                                      uint8_t* __restrict__ img) {
    const int t = blockIdx.x, qb = blockIdx.y, T = gridDim.x;
    uint8_t* dst = img + ((size_t)qb * T + t) * kFp4SlabQ;
    for (int item = threadIdx.x; item < kQB * 8; item += 256) {
        const int row = item >> 3, pos = item & 7;
        const int chunk = strip_chunk(pos, row);
        const int q = qb * kQB + row;
        const int k0 = t * kFp4SlabK + chunk * 32;
        u32x4_t w = {0u, 0u, 0u, 0u};
        if (q < Q) {
            const uint8_t* src = qcodes + (size_t)q * ldq + (k0 >> 1);
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (k0 + 2 * e < D) w[e >> 2] |= ((uint32_t)src[e] & (k0 + 2 * e + 1 < D ? 0xffu : 0x0fu)) << (8 * (e & 3));
        }
        *(u32x4_t*)(dst + row * 128 + pos * 16) = w;
    }
    {
        const int item = threadIdx.x;                   // 256 dwords: 192 of block bytes, 64 of zeros
        uint32_t w = 0;
        if (item < 2 * kQB) {
            const int lhi = item / kQB, q = qb * kQB + item % kQB;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int b = t * 8 + s * 2 + lhi;
                w |= (uint32_t)((q < Q && b * 32 < D) ? qexps[(size_t)q * ldqe + b] : (uint8_t)127) << (8 * s);
            }
        }
        *(uint32_t*)(dst + kFp4SlabCodes + item * 4) = w;
    }
}

__global__ void __launch_bounds__(768) sim_fp4_kernel(const uint8_t* __restrict__ P, int ldp, const uint8_t* __restrict__ PE,
                                                     int ldpe, int NP, int Kb, const uint8_t* __restrict__ img,
                                                     const float* __restrict__ qscales, const float* __restrict__ bscales,
                                                     float* __restrict__ out, int ldo, int NQ, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FlatFrame f(NP);
    const int rot = strip_rot(f.tile, T);

    if (wave >= 8) {
        const int lw = wave - 8;
        // Kb bytes of every row are readable
        const __amdgpu_buffer_rsrc_t rsrc_p = f.database(P, ldp, Kb), rsrc_q = f.image(img, T, kFp4SlabQ);
        const ChunkCutLoader db(lw, lane, (uint32_t)ldp, Kb, T);
        // the image of a slab: 13 pieces; loader 0 takes the block bytes' piece with its three
        const bool four = lw == 0;
        strip_load<kFp4Stage, kFp4Stages, 11, 12>(smem, T, rot, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
#pragma unroll
            for (int i = 0; i < 3; ++i) strip_image_piece(rsrc_q, stage, lw * 3 + i, lane, u * kFp4SlabQ);
            if (four) strip_image_piece(rsrc_q, stage, 12, lane, u * kFp4SlabQ);
        }, four);
        return;
    }

    const StripLane L(wave, lane);
    const int n = f.n(wave, L);
    // the row's block bytes: 8 per slab, one slab ahead (a row past NP reads the last row's; its scores are not stored)
    const uint8_t* erow = PE + (size_t)min(n, NP - 1) * ldpe;
    // byte s of a step's scale dword is block 2 s + lhi of the slab; in the last slab the blocks past Kb hold 127
    const int lastb = (Kb >> 4) - (T - 1) * 8;
    uint32_t pad = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) pad |= (s * 2 + L.lhi >= lastb ? 0xffu : 0u) << (8 * s);
    f32x16_t acc[3] = {};
    u32x2_t nxt = *(const u32x2_t*)(erow + 8 * strip_slab(0, rot, T));
    int t = 0;
    strip_consume<kFp4Stage, kFp4Stages>(smem, T, rot, [&](const char* stage, int u) __attribute__((always_inline)) {
        const u32x2_t cur = nxt;
        if (++t < T) nxt = *(const u32x2_t*)(erow + 8 * strip_slab(t, rot, T));
        uint32_t e = fp4_pick_bytes(cur, L.lhi);
        if (u == T - 1) e = (e & ~pad) | (0x7f7f7f7fu & pad);
        fp4_slab_mma<3>(L, stage, e, acc);
    });

    flat_store(f, L, n, qscales, bscales, out, ldo, NQ, [&](int j, int i, int) __attribute__((always_inline)) { return acc[j][i]; });
}

int similarity_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                   const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, int N, int D,
                   float* scores, int lds, hipStream_t stream) {
    const int Kb = pad64(D) / 2, T = fp4_slabs(D), qblocks = ceil_div(Q, kQB);
    static std::atomic<uint64_t> attr_done{0};
    return flat_scan_launch(
        "similarity_fp4", Q, N, (size_t)qblocks * T * kFp4SlabQ, (const void*)sim_fp4_kernel, kFp4Lds, attr_done, stream,
        [&](char* img) {
            hipLaunchKernelGGL(fp4_image_kernel, dim3(T, qblocks), dim3(256), 0, stream, qcodes, ldq, qexps, ldqe, Q, D, (uint8_t*)img);
            return hipGetLastError();
        },
        [&](char* img, dim3 grid) {
            hipLaunchKernelGGL(sim_fp4_kernel, grid, dim3(768), kFp4Lds, stream, bcodes, ldb, bexps, ldbe, N, Kb, (const uint8_t*)img,
                               qscales, bscales, scores, lds, Q, T);
        });
}

// the scan's admission rules beyond the sizes (c_api.hip reports them): flat_scan_admissible's, and one aligned 8-byte load
// of block bytes per slab
bool similarity_fp4_admissible(const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, int D) {
    return flat_scan_admissible(bcodes, ldb) && (ldbe & 7) == 0 && (((uintptr_t)bexps) & 7) == 0 && ldbe >= fp4_exp_bytes(D);
}

}  // namespace dir

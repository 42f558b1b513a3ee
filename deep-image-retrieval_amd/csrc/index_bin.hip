// index_bin.hip — the binary descriptor index: one sign bit per value and one fp32 scale per row, scanned on the int8
// matrix cores against int8 query codes.
//
// A row of D values is D / 8 bytes of bits (include/dir_engine.h gives the definition): a quarter of the fp4 row, an eighth
// of the int8 row.  The query side stays dir_quantize_rows_i8's, so with s_k = +-1 the sum t = sum_k qc_k s_k is an exact
// int32 of at most 127 * 131072 < 2^24 and
//     scores[q][n] = ((float)t * qscales[q]) * bscales[n]
// is one defined fp32 number whatever the tiling or the chunking, as in the int8 index.  The kernel multiplies the bits
// as 0 / 1 code bytes, t = 2 * sum_k qc_k b_k - sum_k qc_k, the second sum from a small kernel of its own.
//
// sim_bin_kernel runs strip_stream.h's pipeline - one 768-thread workgroup per 256 database rows, eight consumer waves of
// 32 rows against a block of 96 query rows (three i32x16 accumulators of v_mfma_i32_32x32x32_i8), four loader waves that
// only issue LDS-DMA - on TWO rings, because a 128-byte stage row of bits is 1024 k and the int8 query part of a stage that
// wide would be 96 KB:
//   the database ring   three slots of 32 KB, StripLoader's geometry (128 bytes of every row, XOR-swizzled, the last slab
//                       cut by 16-byte chunk): every byte of bits comes from HBM once per query block, in whole 128-byte
//                       pieces of a row;
//   the query ring      four slots of index_i8.hip's 12 KB image of 128 k, re-streamed from L2, eight to a database slab.
// One ring_barrier() per sub-slab of 128 k.  A loader wave issues the same number of LDS-DMA instructions after every
// hand-off - its three pieces of the sub-slab three ahead and, where a row is wider than two slabs, ONE of its eight
// pieces of the slab two ahead - so one vmcnt immediate is the whole bookkeeping; what lies past the end is asked for out
// of range and lands as zeros in a slot nobody reads.  A consumer lane reads its row's 16-byte chunk of the sub-slab once
// and widens 16 bits per MFMA step to code bytes in registers (bin_widen: three VALU operations per dword).  Up to
// D = 2048 (two slabs) the whole strip is resident after the prologue.  No K rotation: a row pitch of 256 bytes makes a
// workgroup's strip one contiguous 64 KB, which spreads over the channels by itself.
#include "dir_common.h"
#include "flat_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the definition is in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kBinMaxDim = 131072;          // 127 * 131072 = 16 646 144 < 2^24: (float)t is exact

int index_bin_max_dim() { return kBinMaxDim; }

// ---- quantisation ------------------------------------------------------------------------------------------------------
// One wave per row, quantize_rows_i8_kernel's walk: lane l owns the quads k = 256 j + 4 l + 0..3, j ascending, and its two
// sums are chains over them in that order; the butterfly then adds lane l ^ d for d = 32, 16, .. 1.  Eight neighbouring
// lanes hold the 32 bits of one dword.  A row of up to 2048 values stays in registers between the sums and the bit pack.
__global__ void __launch_bounds__(256) quantize_rows_bin_kernel(const float* __restrict__ X, int ldx, int N, int D,
                                                              uint8_t* __restrict__ bits, int ldb,
                                                              float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* row = X + (size_t)n * ldx;
    const bool vec = (ldx & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    const int W = bin_row_bytes(D) >> 2;               // dwords written
    const int chunks = (D + 2047) >> 11;
    f32x4_t v[8];
    float sumabs = 0.f, sumsq = 0.f;
    bool bad = false;
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = load4_guarded(row, ((c * 8 + i) * 64 + lane) * 4, D, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = v[i][e];
                const uint32_t b = __builtin_bit_cast(uint32_t, xe) & 0x7fffffffu;
                bad |= b >= 0x7f800000u;                              // an infinity or a NaN
                sumabs = __fadd_rn(sumabs, __builtin_bit_cast(float, b));
                sumsq = __fadd_rn(sumsq, __fmul_rn(xe, xe));
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sumabs = __fadd_rn(sumabs, __shfl_xor(sumabs, d));
        sumsq = __fadd_rn(sumsq, __shfl_xor(sumsq, d));
    }
    bad = __any(bad);
    float scale = __fdiv_rn(sumsq, sumabs);
    const bool zero = bad || !(sumabs > 0.f && sumabs <= 3.4028234663852886e38f && sumsq <= 3.4028234663852886e38f);
    if (zero) scale = bad ? __builtin_nanf("") : 0.f;
    uint32_t* brow = (uint32_t*)(bits + (size_t)n * ldb);
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int w = (c * 8 + i) * 8 + (lane >> 3);              // 32 k to a dword, 4 k to a lane
            if ((c * 8 + i) * 8 >= W) continue;                       // (wave-uniform: the shuffles below see all lanes)
            const int k = ((c * 8 + i) * 64 + lane) * 4;
            if (chunks > 1) v[i] = load4_guarded(row, k, D, vec);
            uint32_t word = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = v[i][e];
                const bool on = !zero && k + e < D && (__builtin_bit_cast(uint32_t, xe) >> 31) == 0u;
                word |= (uint32_t)on << (4 * (lane & 7) + e);
            }
            word |= (uint32_t)__shfl_xor((int)word, 1);
            word |= (uint32_t)__shfl_xor((int)word, 2);
            word |= (uint32_t)__shfl_xor((int)word, 4);
            if ((lane & 7) == 0 && w < W) brow[w] = word;             // (ldb % 4 == 0, bits 4-byte aligned)
        }
    }
    if (lane == 0) scales[n] = scale;
}

int quantize_rows_bin(const float* X, int ldx, int N, int D, uint8_t* bits, int ldb, float* scales, hipStream_t stream) {
    return rows_launch("quantize_rows_bin", "N", N, [&](unsigned blocks) {
        hipLaunchKernelGGL(quantize_rows_bin_kernel, dim3(blocks), dim3(256), 0, stream, X, ldx, N, D, bits, ldb, scales);
    });
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// qsum[q] = sum_{k < D} qcodes[q][k] for the rows of the query blocks (zero past Q): one wave per row.
__global__ void __launch_bounds__(256) code_sums_kernel(const int8_t* __restrict__ qcodes, int ldq, int Q, int D, int rows,
                                                      int* __restrict__ qsum) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= rows) return;
    int s = 0;
    if (q < Q)
        for (int k = lane; k < D; k += 64) s += qcodes[(size_t)q * ldq + k];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) qsum[q] = s;
}

// the sums of Q rows for a caller that keeps them (the list scan of ivf_bin.hip takes them as an argument)
int code_sums(const int8_t* qcodes, int ldq, int Q, int D, int* qsums, hipStream_t stream) {
    return rows_launch("code_sums", "Q", Q, [&](unsigned blocks) {
        hipLaunchKernelGGL(code_sums_kernel, dim3(blocks), dim3(256), 0, stream, qcodes, ldq, Q, D, Q, qsums);
    });
}

// S sub-slabs of 128 k = the 16-byte chunks of a row of bits; T = ceil(S / 8) database slabs.
// STREAM: rows wider than two slabs - the database ring turns, one piece per loader and hand-off.
template <bool STREAM>
__device__ __forceinline__ void bin_load(char* smem, int lw, int lane, __amdgpu_buffer_rsrc_t rsrc_p,
                                         __amdgpu_buffer_rsrc_t rsrc_q, const ChunkCutLoader& db, int S, int T) {
    constexpr int OPS = STREAM ? 4 : 3;                // LDS-DMA instructions of this wave after every hand-off
    auto lim = [&](int u) __attribute__((always_inline)) {
        return u < db.last ? 8u : u == db.last ? (uint32_t)db.keep : 0u;
    };
    // sub-slab s into its slot: this loader's three of the twelve pieces (past S: out of range, zeros into a free slot)
    auto put_q = [&](int s) __attribute__((always_inline)) {
        char* dst = smem + kBinQOff + (s % kBinQStages) * kBinSub;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int p = lw * 3 + i;
            dma16(rsrc_q, dst + p * kStripPiece, s < S ? (uint32_t)(p * kStripPiece + lane * 16) : kOOB, s * kBinSub);
        }
    };
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const uint32_t l = lim(u);
#pragma unroll
        for (int i = 0; i < 8; ++i) db.piece(rsrc_p, smem + u * kStripSlab, u, i, l);
    }
#pragma unroll
    for (int s = 0; s < kBinQStages - 1; ++s) put_q(s);
    for (int s0 = 0; s0 < S; s0 += 8) {
        const int u = (s0 >> 3) + 2;                   // the slab two ahead, into the slot of the slab everyone has left
        char* slot = smem + (u % kBinDbStages) * kStripSlab;
        const uint32_t l = lim(u);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int s = s0 + i;
            if (s >= S) break;
            // sub-slab s (issued after hand-off s - 3, behind every piece of its database slab) has landed when at most
            // the instructions of the last two hand-offs are in flight; before hand-off 0 and 1 those are sub-slabs 1, 2
            if (STREAM && s >= 2)
                wait_vmcnt<2 * OPS>();
            else
                wait_vmcnt<6>();
            ring_barrier();   // hand-off s: sub-slab s is complete; the consumers have left sub-slab s - 1
            if (STREAM) db.piece(rsrc_p, slot, u, i, l);
            put_q(s + kBinQStages - 1);
        }
    }
}

__global__ void __launch_bounds__(768) sim_bin_kernel(const uint8_t* __restrict__ P, int ldp, int NP, int Kb,
                                                     const int8_t* __restrict__ img, const int* __restrict__ qsum,
                                                     const float* __restrict__ qscales, const float* __restrict__ bscales,
                                                     float* __restrict__ out, int ldo, int NQ, int S, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FlatFrame f(NP);

    if (wave >= 8) {
        const int lw = wave - 8;
        // Kb bytes of every row are readable
        const __amdgpu_buffer_rsrc_t rsrc_p = f.database(P, ldp, Kb), rsrc_q = f.image(img, S, kBinSub);
        const ChunkCutLoader db(lw, lane, (uint32_t)ldp, Kb, T);
        if (T > 2)
            bin_load<true>(smem, lw, lane, rsrc_p, rsrc_q, db, S, T);
        else
            bin_load<false>(smem, lw, lane, rsrc_p, rsrc_q, db, S, T);
        return;
    }

    const StripLane L(wave, lane);
    i32x16_t acc[3] = {};
    for (int s = 0; s < S; ++s) {
        ring_barrier();   // hand-off s (see bin_load)
        bin_sub_mma<3>(L, smem + ((s >> 3) % kBinDbStages) * kStripSlab, s & 7, smem + kBinQOff + (s % kBinQStages) * kBinSub, acc);
    }

    flat_store(f, L, f.n(wave, L), qscales, bscales, out, ldo, NQ, [&](int j, int i, int q) __attribute__((always_inline)) {
        return (float)(2 * acc[j][i] - qsum[q]);
    });
}

int similarity_bin(const int8_t* qcodes, int ldq, const float* qscales, int Q, const uint8_t* bits, int ldb,
                   const float* bscales, int N, int D, float* scores, int lds, hipStream_t stream) {
    const int Kb = bin_row_bytes(D), S = Kb / 16, T = ceil_div(S, 8), qblocks = ceil_div(Q, kQB);
    // stream-ordered scratch: the query image, then the query sums of whole blocks
    const size_t img_bytes = (size_t)qblocks * S * kBinSub;
    static std::atomic<uint64_t> attr_done{0};
    return flat_scan_launch(
        "similarity_bin", Q, N, img_bytes + (size_t)qblocks * kQB * sizeof(int), (const void*)sim_bin_kernel, kBinLds, attr_done,
        stream,
        [&](char* img) {
            const hipError_t e = code_image(qcodes, ldq, Q, D, (int8_t*)img, S, qblocks, stream);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(code_sums_kernel, dim3(qblocks * kQB / 4), dim3(256), 0, stream, qcodes, ldq, Q, D, qblocks * kQB,
                               (int*)(img + img_bytes));
            return hipGetLastError();
        },
        [&](char* img, dim3 grid) {
            hipLaunchKernelGGL(sim_bin_kernel, grid, dim3(768), kBinLds, stream, bits, ldb, N, Kb, (const int8_t*)img,
                               (const int*)(img + img_bytes), qscales, bscales, scores, lds, Q, S, T);
        });
}

}  // namespace dir

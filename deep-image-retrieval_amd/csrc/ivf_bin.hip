// ivf_bin.hip — the inverted file over sign-bit rows: the scan of the probed lists on the int8 matrix cores.
//
// index_bin.hip keeps 260 bytes a row of 2048 and reads all of them; ivf.hip reads only the lists a query falls into.
// ivf_scan_bin_kernel is ivf_scan_i8_kernel's cut - list-major, a workgroup takes up to 256 consecutive rows of ONE list
// against a group of up to 32 of the queries that probe it, the same probe tables, the same work items, the same early
// returns and scattered epilogue - with sim_bin_kernel's arithmetic: a 128-byte stage row of bits is 1024 k, a lane widens
// 16 bits to 16 code bytes of 0 / 1 per v_mfma_i32_32x32x32_i8 step (bin_sub_mma<1>, one i32x16 accumulator block), and the
// epilogue forms t = 2 * acc - qsum[q], an exact int32, so a score is dir_similarity_bin's number whatever the cut.
//
// ONE ring.  The flat scan rides on two because its 96 query rows x 1024 k are 96 KB a stage.  A group of 32 rows x 1024 k
// of int8 codes is 32 KB, the size of the database slab of the same k, so a stage here is simply both:
//   [0, 32768)             the database slab: 256 rows x 128 bytes, ChunkCutLoader's pieces, the last slab cut by 16-byte chunk;
//   [32768 + c * 4096, ..) query sub-image c = 0 .. 7: 32 rows x 128 bytes of k = 1024 u + 128 c + 0 .. 127, swizzled like
//                          the database rows - the layout bin_sub_mma reads.
// Two stages of 64 KB, strip_load / strip_consume as they stand: one ring_barrier() per 1024 k where the flat kernel has
// one per 128 k.  Up to D = 2048 (two slabs) no slot is used twice: the loaders never wait for a consumer.  A loader wave
// issues 16 LDS-DMA instructions a slab - its eight database pieces and its piece (rows 8 lw .. 8 lw + 7) of each of the
// eight sub-images, the query rows gathered where they lie by a per-lane row offset from the pair table (kOOB for an
// empty row of the group).  A query chunk at or past pad64(D) bytes of its row is asked for out of range: the query pitch
// need not cover a slab, so an uncut lane would read the next query's codes.  The count of instructions stays the same
// for every slab.  The consumers walk only the sub-slabs of the last slab that exist.  No K rotation: a row pitch of 256
// bytes makes a workgroup's strip one contiguous 64 KB, which spreads over the channels by itself.
// LDS: 2 stages x 65 536 = 131 072 of 163 840 bytes.  No atomics, no scratch.
#include "dir_common.h"
#include "ivf_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kIvfBinStage = kStripSlab + 8 * kIvfSub;   // 65536: 1024 k of both operands
static constexpr int kIvfBinStages = 2;
static constexpr int kIvfBinLds = kIvfBinStages * kIvfBinStage;    // 131072 of 163840

// The work item, the query gather and the epilogue: ivf_scan.h.
// Kp: bytes of query codes in a row (pad64(D)); Kb: bytes of bits in a row; S = Kb / 16 sub-slabs, T = ceil(S / 8) slabs.
__global__ void __launch_bounds__(768) ivf_scan_bin_kernel(const int8_t* __restrict__ qcodes, int ldq, const float* __restrict__ qscales,
                                                          const int* __restrict__ qsums, int Q, const uint8_t* __restrict__ P,
                                                          int ldp, const float* __restrict__ bscales, const int* __restrict__ ids,
                                                          int NP, int Kp, int Kb, int S, int T, const int* __restrict__ list_off,
                                                          int nlist, const int* __restrict__ pair_off, const int* __restrict__ pair_q,
                                                          const int* __restrict__ pair_col, const int* __restrict__ item_off,
                                                          float* __restrict__ out, int* __restrict__ out_ids, int ldo, int width) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const IvfItem it(blockIdx.x, item_off, nlist, pair_off, list_off, NP);
    if (!it.valid) return;

    if (wave >= 8) {
        const int lw = wave - 8;
        const __amdgpu_buffer_rsrc_t rsrc_p = buffer_rsrc(P + (size_t)it.i0 * ldp, (uint32_t)(((size_t)it.rows - 1) * ldp + Kb));
        const __amdgpu_buffer_rsrc_t rsrc_q = buffer_rsrc(qcodes, (uint32_t)(((size_t)Q - 1) * ldq + Kp));
        const ChunkCutLoader db(lw, lane, (uint32_t)ldp, Kb, T);
        const IvfQueryLane qs(it, pair_q, Q, ldq, Kp, lw, lane);
        strip_load<kIvfBinStage, kIvfBinStages, 16>(smem, T, 0, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
#pragma unroll
            for (int c = 0; c < 8; ++c)      // sub-image c: bytes u * 1024 + c * 128 .. + 127 of the query rows
                qs.issue(rsrc_q, stage + kStripSlab + c * kIvfSub, u * (8 * kStripRow) + c * kStripRow);
        });
        return;
    }

    const StripLane L(wave, lane);
    i32x16_t acc[1] = {};
    strip_consume<kIvfBinStage, kIvfBinStages>(smem, T, 0, [&](const char* stage, int u) __attribute__((always_inline)) {
        const int subs = min(8, S - 8 * u);                                    // the sub-slabs of this slab that exist
        if (subs == 8) {                                                       // a whole slab: unrolled, the reads run ahead
#pragma unroll
            for (int c = 0; c < 8; ++c) bin_sub_mma<1>(L, stage, c, stage + kStripSlab + c * kIvfSub, acc);
        } else {
            for (int c = 0; c < subs; ++c) bin_sub_mma<1>(L, stage, c, stage + kStripSlab + c * kIvfSub, acc);
        }
    });
    ivf_scatter<true>(it, L, it.r(wave, L), pair_q, pair_col, qscales, qsums, Q, bscales, ids, out, out_ids, ldo, width,
                      [&](int j, int su) __attribute__((always_inline)) { return (float)(2 * acc[0][j] - su); });
}

int ivf_scan_bin(const int8_t* qcodes, int ldq, const float* qscales, const int* qsums, int Q, const uint8_t* bits, int ldb,
                 const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                 const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                 int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    DIR_CHECK(ivf_scan_begin("ivf_scan_bin", Q, width, items, out_ids, lds, stream));
    if (items <= 0 || N <= 0) return DIR_OK;
    const int Kp = pad64(D), Kb = bin_row_bytes(D), S = Kb / 16, T = ceil_div(S, 8);
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_scan_bin_kernel, kIvfBinLds, attr_done));
    hipLaunchKernelGGL(ivf_scan_bin_kernel, dim3((unsigned)items), dim3(768), kIvfBinLds, stream, qcodes, ldq, qscales, qsums, Q,
                       bits, ldb, bscales, ids, N, Kp, Kb, S, T, list_off, nlist, pair_off, pair_q, pair_col, item_off, scores,
                       out_ids, lds, width);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir

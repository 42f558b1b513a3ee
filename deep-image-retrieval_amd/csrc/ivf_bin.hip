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
//   [0, 32768)             the database slab: 256 rows x 128 bytes, Fp4Loader's pieces, the last slab cut by 16-byte chunk;
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
#include "strip_stream.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kIvfBinQG = 32;                    // query rows per group = one 32 x 32 accumulator block
static constexpr int kIvfBinSub = kIvfBinQG * kStripRow;   // 4096: the query sub-image of 128 k
static constexpr int kIvfBinStage = kStripSlab + 8 * kIvfBinSub;   // 65536: 1024 k of both operands
static constexpr int kIvfBinStages = 2;
static constexpr int kIvfBinLds = kIvfBinStages * kIvfBinStage;    // 131072 of 163840

__host__ __device__ inline int ivf_bin_row_bytes(int D) { return ((D + 127) >> 7) * 16; }   // D rounded up to 128, in bits

__global__ void __launch_bounds__(256) fill_ids_bin_kernel(int* __restrict__ out_ids, int lds, int width, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out_ids[(i / width) * lds + (i % width)] = -1;
}

// Workgroup b serves list l with item_off[l] <= b < item_off[l + 1]; its place there is tile * groups + group (ivf.hip).
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
    const int bid = blockIdx.x;
    // the list of this workgroup: the last l with item_off[l] <= bid (uniform: every wave takes the same way out)
    int lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (item_off[mid] <= bid) lo = mid; else hi = mid;
    }
    const int l = lo;
    const int p0 = pair_off[l], p1 = pair_off[l + 1];
    const int groups = (p1 - p0 + kIvfBinQG - 1) / kIvfBinQG;
    const int local = bid - item_off[l];
    if (groups <= 0 || local < 0) return;
    const int tile = local / groups, grp = local - tile * groups;
    const int i0 = list_off[l] + tile * kStripRows;
    const int iend = min(list_off[l + 1], NP);
    const int rows = min(kStripRows, iend - i0);
    const int pbase = p0 + grp * kIvfBinQG;
    if (i0 < 0 || rows <= 0) return;

    if (wave >= 8) {
        const int lw = wave - 8;
        const __amdgpu_buffer_rsrc_t rsrc_p = buffer_rsrc(P + (size_t)i0 * ldp, (uint32_t)(((size_t)rows - 1) * ldp + Kb));
        const __amdgpu_buffer_rsrc_t rsrc_q = buffer_rsrc(qcodes, (uint32_t)(((size_t)Q - 1) * ldq + Kp));
        const Fp4Loader db(lw, lane, (uint32_t)ldp, Kb, T);
        // query piece lw = rows 8 lw .. 8 lw + 7 of the group: row r is the query of pair pbase + r, gathered where it lies
        const int qrow = strip_piece_row(lw, lane), qchunk = strip_piece_chunk(lw, lane);
        uint32_t qvoff = kOOB;                                                 // an empty row of the group reads zeros
        if (pbase + qrow < p1) {
            const int q = pair_q[pbase + qrow];
            if ((unsigned)q < (unsigned)Q) qvoff = (uint32_t)q * (uint32_t)ldq + (uint32_t)qchunk * 16u;
        }
        strip_load<kIvfBinStage, kIvfBinStages, 16>(smem, T, 0, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
            // the lane's chunk of sub-image c is bytes u * 1024 + c * 128 + qchunk * 16 .. + 15 of the query row: past Kp it
            // would be the next query's codes (the scalar offset takes no part in the range check)
            const int left = Kp - u * (8 * kStripRow) - qchunk * 16;           // > 0 where chunk qchunk of sub-image 0 exists
#pragma unroll
            for (int c = 0; c < 8; ++c)
                dma16(rsrc_q, stage + kStripSlab + c * kIvfBinSub + lw * kStripPiece, c * kStripRow >= left ? kOOB : qvoff,
                      u * (8 * kStripRow) + c * kStripRow);
        });
        return;
    }

    const StripLane L(wave, lane);
    i32x16_t acc[1] = {};
    strip_consume<kIvfBinStage, kIvfBinStages>(smem, T, 0, [&](const char* stage, int u) __attribute__((always_inline)) {
        const int subs = min(8, S - 8 * u);                                    // the sub-slabs of this slab that exist
        if (subs == 8) {                                                       // a whole slab: unrolled, the reads run ahead
#pragma unroll
            for (int c = 0; c < 8; ++c) bin_sub_mma<1>(L, stage, c, stage + kStripSlab + c * kIvfBinSub, acc);
        } else {
            for (int c = 0; c < subs; ++c) bin_sub_mma<1>(L, stage, c, stage + kStripSlab + c * kIvfBinSub, acc);
        }
    });

    // scattered epilogue: the lane's 16 pairs are the group rows L.qrow(0, g) + e
    const int r = tile * kStripRows + wave * 32 + L.lrow;    // the row's place in its list
    const int n = list_off[l] + r;
    if (n < iend) {
        const float sb = bscales[n];
        const int id = ids[n];
        // the 16 pairs of this lane in three rounds of independent loads (query, column; scale and sum; then the stores)
        int qv[16];
        long cv[16];
        float sq[16];
        int su[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int pi = pbase + L.qrow(0, j >> 2) + (j & 3);
            const bool ok = pi < p1;
            qv[j] = ok ? pair_q[pi] : -1;
            cv[j] = ok ? (long)pair_col[pi] + r : -1;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((unsigned)qv[j] >= (unsigned)Q || cv[j] >= width) cv[j] = -1;        // a table that does not fit: no store
            sq[j] = cv[j] >= 0 ? qscales[qv[j]] : 0.f;
            su[j] = cv[j] >= 0 ? qsums[qv[j]] : 0;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (cv[j] >= 0) {
                const int t = 2 * acc[0][j] - su[j];
                out[(size_t)qv[j] * ldo + cv[j]] = __fmul_rn(__fmul_rn((float)t, sq[j]), sb);
                out_ids[(size_t)qv[j] * ldo + cv[j]] = id;
            }
    }
}

// the scan's admission rules beyond the sizes (c_api.hip reports them): 16-byte pieces, one 2 GB descriptor per operand
bool ivf_scan_bin_admissible(const int8_t* qcodes, int ldq, int Q, const uint8_t* bits, int ldb) {
    return ((ldq | ldb) & 15) == 0 && ((((uintptr_t)qcodes) | ((uintptr_t)bits)) & 15) == 0 &&
           (size_t)ldb * kStripRows < (1ull << 31) && (size_t)ldq * (size_t)(Q > 0 ? Q : 1) < (1ull << 31);
}

int ivf_scan_bin(const int8_t* qcodes, int ldq, const float* qscales, const int* qsums, int Q, const uint8_t* bits, int ldb,
                 const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                 const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                 int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    const long total = (long)Q * width;
    // (refused, not cut: as in ivf_scan_i8, Q * width >= 2^32 means score and id rows of 32 GiB for one chunk)
    if (!launch_fits((total + 255) / 256, 256))
        return fail(DIR_ERR_INVALID, "ivf_scan_bin: Q * width must stay below 2^32 (one thread per id slot): cut the queries");
    if (!launch_fits(items, 768))
        return fail(DIR_ERR_INVALID, "ivf_scan_bin: items * 768 must stay below 2^32 (768 threads per item): cut the queries");
    hipLaunchKernelGGL(fill_ids_bin_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out_ids, lds, width, total);
    DIR_HIP_CHECK(hipGetLastError());
    if (items <= 0 || N <= 0) return DIR_OK;
    const int Kp = pad64(D), Kb = ivf_bin_row_bytes(D), S = Kb / 16, T = ceil_div(S, 8);
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_scan_bin_kernel, kIvfBinLds, attr_done));
    hipLaunchKernelGGL(ivf_scan_bin_kernel, dim3((unsigned)items), dim3(768), kIvfBinLds, stream, qcodes, ldq, qscales, qsums, Q,
                       bits, ldb, bscales, ids, N, Kp, Kb, S, T, list_off, nlist, pair_off, pair_q, pair_col, item_off, scores,
                       out_ids, lds, width);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir

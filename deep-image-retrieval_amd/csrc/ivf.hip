// ivf.hip — the inverted-file int8 index: the sums of a k-means step and the scan of the probed lists.
//
// An inverted file keeps the int8 database of index_i8.hip grouped by the list (k-means cell) of every row and scans,
// for a query, only the `nprobe` lists whose centroids score best.  Scoring the centroids, ranking them and ranking the
// candidates are dir_similarity_i8 / dir_topk as they stand; two things are new:
//
// segment_sums_kernel - the sums of a Lloyd iteration: sums[s] = the rows order[seg_off[s] .. seg_off[s+1]) of X added up
//   in fp32 in a FIXED order (no atomics: their arrival order would make a training run irreproducible).
//
// ivf_scan_i8_kernel - strip_stream.h's pipeline as sim_i8_kernel runs it (K slabs of 128 codes, int32 accumulators, the
//   same two-multiply epilogue: the scores are dir_similarity_i8's numbers) with FOUR stages and cut LIST-MAJOR: a
//   workgroup takes up to 256 consecutive rows of ONE list and multiplies them against a group of up to 32 of the queries
//   that probe that list, so a batch of queries that share a list reads it once.  (Cut query-major, one workgroup per
//   (query, list), a batch reads Q * nprobe / nlist of the database: at 70 queries and 16 of 1024 lists more bytes than the
//   flat scan.)  Why 32 queries and not sim_i8_kernel's 96: a list is probed by Q * nprobe / nlist queries on average - a
//   handful - so two of three accumulator blocks would multiply zeros, and the 8 KB of LDS per stage that a 96-row query
//   image costs buy a fourth stage instead (three slabs, 108 KB, in flight per CU: with one query the grid is a few dozen
//   workgroups and the bytes in flight per workgroup are the speed).  A list probed by more than 32 queries takes further
//   groups, each of which reads the tile again (from L2, the groups of a tile are neighbours in the grid).
//   The query rows of a group are gathered straight from the query codes by the loader lanes - a per-lane row offset
//   from the pair table, out-of-range for the empty rows of a group - the way the database pieces are addressed; no stage
//   image is written per list.
#include "dir_common.h"
#include "ivf_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

// ---- segment sums ------------------------------------------------------------------------------------------------------
// One workgroup of four waves per (256 columns, segment); a lane owns four consecutive columns.  Wave w adds the rows
// seg_off[s] + w, + 4, ... of the segment into four chains (row j of the wave goes to chain j % 4), folds them as
// (c0 + c1) + (c2 + c3), and the four waves' partial sums are folded the same way through LDS: the order is a function
// of the segment's length alone.  n / 16 + 4 additions on the longest path.
static constexpr int kSegCols = 256;

__global__ void __launch_bounds__(256) segment_sums_kernel(const float* __restrict__ X, int ldx, int N, int D,
                                                         const int* __restrict__ order, const int* __restrict__ seg_off,
                                                         float* __restrict__ sums, int lds) {
    __shared__ f32x4_t part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = blockIdx.y;
    const int k = blockIdx.x * kSegCols + lane * 4;
    const int i0 = seg_off[s], i1 = seg_off[s + 1];
    const bool vec = (ldx & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    f32x4_t c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    if (k < D) {
        for (int i = i0 + wave; i < i1; i += 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ii = i + 4 * j;
                if (ii < i1) {
                    const int r = order[ii];
                    if ((unsigned)r < (unsigned)N) c[j] += load4_guarded(X + (size_t)r * ldx, k, D, vec);
                }
            }
        }
    }
    part[wave][lane] = (c[0] + c[1]) + (c[2] + c[3]);
    __syncthreads();
    if (wave == 0 && k < D) {
        const f32x4_t t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        float* dst = sums + (size_t)s * lds + k;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k + e < D) dst[e] = t[e];
    }
}

int segment_sums(const float* X, int ldx, int N, int D, const int* order, const int* seg_off, int S, float* sums, int lds,
                 hipStream_t stream) {
    if (S <= 0) return DIR_OK;
    if (S > kMaxGridYZ) return fail(DIR_ERR_INVALID, "segment_sums: more than 65535 segments");
    hipLaunchKernelGGL(segment_sums_kernel, dim3((unsigned)ceil_div(D, kSegCols), (unsigned)S), dim3(256), 0, stream, X, ldx, N,
                       D, order, seg_off, sums, lds);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the scan of the probed lists --------------------------------------------------------------------------------------
static constexpr int kIvfStage = kStripSlab + kIvfSub;   // 36864
static constexpr int kIvfStages = 4;                // three slabs in flight, one being multiplied
static constexpr int kIvfLds = kIvfStages * kIvfStage;   // 147456 of 163840

__global__ void __launch_bounds__(256) fill_ids_kernel(int* __restrict__ out_ids, int lds, int width, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out_ids[(i / width) * lds + (i % width)] = -1;
}

// The work item, the query gather and the epilogue: ivf_scan.h.
__global__ void __launch_bounds__(768) ivf_scan_i8_kernel(const int8_t* __restrict__ qcodes, int ldq, const float* __restrict__ qscales,
                                                         int Q, const int8_t* __restrict__ P, int ldp,
                                                         const float* __restrict__ bscales, const int* __restrict__ ids, int NP,
                                                         int Kp, int T, const int* __restrict__ list_off, int nlist,
                                                         const int* __restrict__ pair_off, const int* __restrict__ pair_q,
                                                         const int* __restrict__ pair_col, const int* __restrict__ item_off,
                                                         float* __restrict__ out, int* __restrict__ out_ids, int ldo, int width) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bid = blockIdx.x;
    const IvfItem it(bid, item_off, nlist, pair_off, list_off, NP);
    if (!it.valid) return;
    const int rot = strip_rot(bid, T);

    if (wave >= 8) {
        const int lw = wave - 8;
        const __amdgpu_buffer_rsrc_t rsrc_p = buffer_rsrc(P + (size_t)it.i0 * ldp, (uint32_t)(((size_t)it.rows - 1) * ldp + Kp));
        const __amdgpu_buffer_rsrc_t rsrc_q = buffer_rsrc(qcodes, (uint32_t)(((size_t)Q - 1) * ldq + Kp));
        const StripLoader<true> db(lw, lane, (uint32_t)ldp, Kp, T);
        const IvfQueryLane qs(it, pair_q, Q, ldq, Kp, lw, lane);
        strip_load<kIvfStage, kIvfStages, 9>(smem, T, rot, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
            qs.issue(rsrc_q, stage + kStripSlab, u * kStripRow);
        });
        return;
    }

    const StripLane L(wave, lane);
    i32x16_t acc[1] = {};
    strip_consume<kIvfStage, kIvfStages>(smem, T, rot, [&](const char* stage, int) __attribute__((always_inline)) {
        code_slab_mma<1>(L, stage, acc);
    });
    ivf_scatter<false>(it, L, it.r(wave, L), pair_q, pair_col, qscales, nullptr, Q, bscales, ids, out, out_ids, ldo, width,
                       [&](int j, int) __attribute__((always_inline)) { return (float)acc[0][j]; });
}

// the scans' admission rule beyond the sizes (c_api.hip reports it): 16-byte pieces, one 2 GB descriptor per operand
bool ivf_scan_admissible(const void* qcodes, int ldq, int Q, const void* bcodes, int ldb) {
    return ((ldq | ldb) & 15) == 0 && ((((uintptr_t)qcodes) | ((uintptr_t)bcodes)) & 15) == 0 &&
           (size_t)ldb * kStripRows < (1ull << 31) && (size_t)ldq * (size_t)(Q > 0 ? Q : 1) < (1ull << 31);
}

// What a list-major scan does before its kernel: the two launch extents (refused, not cut: a caller reaches Q * width >=
// 2^32 only with score and id rows of 32 GiB for one chunk), then id -1 in every slot.  `who`: the entry, for the message.
int ivf_scan_begin(const char* who, long Q, int width, int items, int* out_ids, int lds, hipStream_t stream) {
    const long total = Q * width;
    if (!launch_fits((total + 255) / 256, 256))
        return fail(DIR_ERR_INVALID, std::string(who) + ": Q * width must stay below 2^32 (one thread per id slot): cut the queries");
    if (!launch_fits(items, 768))
        return fail(DIR_ERR_INVALID, std::string(who) + ": items * 768 must stay below 2^32 (768 threads per item): cut the queries");
    hipLaunchKernelGGL(fill_ids_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out_ids, lds, width, total);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

int ivf_scan_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    DIR_CHECK(ivf_scan_begin("ivf_scan_i8", Q, width, items, out_ids, lds, stream));
    if (items <= 0 || N <= 0) return DIR_OK;
    const int Kp = pad64(D), T = ceil_div(Kp, kStripRow);
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_scan_i8_kernel, kIvfLds, attr_done));
    hipLaunchKernelGGL(ivf_scan_i8_kernel, dim3((unsigned)items), dim3(768), kIvfLds, stream, qcodes, ldq, qscales, Q, bcodes,
                       ldb, bscales, ids, N, Kp, T, list_off, nlist, pair_off, pair_q, pair_col, item_off, scores, out_ids,
                       lds, width);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir

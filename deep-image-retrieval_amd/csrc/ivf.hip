// ivf.hip — the inverted-file int8 index: the sums of a k-means step and the scan of the probed lists.
//
// An inverted file keeps the int8 database of index_i8.hip grouped by the list (k-means cell) of every row and scans,
// for a query, only the `nprobe` lists whose centroids score best.  Scoring the centroids, ranking them and ranking the
// candidates are dir_similarity_i8 / dir_topk as they stand; two things are new:
//
// segment_sums_kernel - the sums of a Lloyd iteration: sums[s] = the rows order[seg_off[s] .. seg_off[s+1]) of X added up
//   in fp32 in a FIXED order (no atomics: their arrival order would make a training run irreproducible).
//
// ivf_scan_i8_kernel - sim_i8_kernel's pipeline (LDS-DMA loader waves, consumer waves on v_mfma_i32_32x32x32_i8, K slabs of
//   128, int32 accumulators, the same two-multiply epilogue: the scores are dir_similarity_i8's numbers) cut LIST-MAJOR: a
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
#include "conv_device.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(16))) int i32x16_t;

// ---- segment sums ------------------------------------------------------------------------------------------------------
// One workgroup of four waves per (256 columns, segment); a lane owns four consecutive columns.  Wave w adds the rows
// seg_off[s] + w, + 4, ... of the segment into four chains (row j of the wave goes to chain j % 4), folds them as
// (c0 + c1) + (c2 + c3), and the four waves' partial sums are folded the same way through LDS: the order is a function
// of the segment's length alone.  n / 16 + 4 additions on the longest path.
static constexpr int kSegCols = 256;

__device__ __forceinline__ f32x4_t seg_load4(const float* __restrict__ row, int k, int D, bool vec) {
    f32x4_t v = {0.f, 0.f, 0.f, 0.f};
    if (vec && k + 3 < D) return *(const f32x4_t*)(row + k);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (k + e < D) v[e] = row[k + e];
    return v;
}

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
                    if ((unsigned)r < (unsigned)N) c[j] += seg_load4(X + (size_t)r * ldx, k, D, vec);
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
    if (S > 65535) return fail(DIR_ERR_INVALID, "segment_sums: more than 65535 segments");
    hipLaunchKernelGGL(segment_sums_kernel, dim3((unsigned)ceil_div(D, kSegCols), (unsigned)S), dim3(256), 0, stream, X, ldx, N,
                       D, order, seg_off, sums, lds);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the scan of the probed lists --------------------------------------------------------------------------------------
static constexpr int kIvfQG = 32;                   // query rows per group = one 32 x 32 accumulator block
static constexpr int kIvfRows = 256;                // database rows per workgroup
static constexpr int kIvfSlabK = 128;               // k per slab = bytes per stage row
static constexpr int kIvfSlabP = kIvfRows * 128;    // 32768
static constexpr int kIvfSlabQ = kIvfQG * 128;      // 4096
static constexpr int kIvfStage = kIvfSlabP + kIvfSlabQ;
static constexpr int kIvfStages = 4;                // three slabs in flight, one being multiplied
static constexpr int kIvfLds = kIvfStages * kIvfStage;   // 147456 of 163840

__global__ void __launch_bounds__(256) fill_ids_kernel(int* __restrict__ out_ids, int lds, int width, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < total) out_ids[(i / width) * lds + (i % width)] = -1;
}

// Workgroup b serves list l with item_off[l] <= b < item_off[l + 1]; its place there is tile * groups + group, groups =
// the 32-pair groups of the list.  pair_off [nlist + 1] is the CSR of the (query, slot) pairs by list, pair_q / pair_col
// the query and the first output column of every pair.
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
    // the list of this workgroup: the last l with item_off[l] <= bid (uniform: every wave takes the same way out)
    int lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (item_off[mid] <= bid) lo = mid; else hi = mid;
    }
    const int l = lo;
    const int p0 = pair_off[l], p1 = pair_off[l + 1];
    const int groups = (p1 - p0 + kIvfQG - 1) / kIvfQG;
    const int local = bid - item_off[l];
    if (groups <= 0 || local < 0) return;
    const int tile = local / groups, grp = local - tile * groups;
    const int i0 = list_off[l] + tile * kIvfRows;
    const int iend = min(list_off[l + 1], NP);
    const int rows = min(kIvfRows, iend - i0);
    const int pbase = p0 + grp * kIvfQG;
    if (i0 < 0 || rows <= 0) return;
    const int rot = (int)(((unsigned)bid * 7u) % (unsigned)T);

    if (wave >= 8) {
        // ================================ loaders ==============================================================
        const int lw = wave - 8;
        const __amdgpu_buffer_rsrc_t rsrc_p = buffer_rsrc(P + (size_t)i0 * ldp, (uint32_t)(((size_t)rows - 1) * ldp + Kp));
        const __amdgpu_buffer_rsrc_t rsrc_q = buffer_rsrc(qcodes, (uint32_t)(((size_t)Q - 1) * ldq + Kp));
        uint32_t pvoff[8];
        uint32_t upper = 0;      // bit i: this lane's chunk of piece i lies in the upper 64 bytes of a slab
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = (lw * 8 + i) * 8 + (lane >> 3);
            const int chunk = (lane & 7) ^ ((row >> 1) & 7);
            pvoff[i] = (uint32_t)row * (uint32_t)ldp + (uint32_t)chunk * 16u;   // rows past `rows`: out of range -> 0
            upper |= (uint32_t)(chunk >= 4) << i;
        }
        // query piece lw = rows 8 lw .. 8 lw + 7 of the group: row r is the query of pair pbase + r, gathered where it lies
        const int qrow = lw * 8 + (lane >> 3);
        const int qchunk = (lane & 7) ^ ((qrow >> 1) & 7);
        uint32_t qvoff = kOOB;                                                 // an empty row of the group reads zeros
        if (pbase + qrow < p1) {
            const int q = pair_q[pbase + qrow];
            if ((unsigned)q < (unsigned)Q) qvoff = (uint32_t)q * (uint32_t)ldq + (uint32_t)qchunk * 16u;
        }
        const bool qupper = qchunk >= 4;
        // Kp % 128 == 64: the upper half of the last slab lies past Kp.  The scalar offset takes no part in the range
        // check, so those lanes ask for an address that is out of range by itself.
        const bool half = (Kp & 64) != 0;
        auto issue = [&](int t) __attribute__((always_inline)) {
            int u = t + rot;
            u = u >= T ? u - T : u;
            char* stage = smem + (t % kIvfStages) * kIvfStage;
            const bool cut = half && u == T - 1;
#pragma unroll
            for (int i = 0; i < 8; ++i)
                dma16(rsrc_p, stage + (lw * 8 + i) * 1024, (cut && ((upper >> i) & 1u)) ? kOOB : pvoff[i], u * kIvfSlabK);
            dma16(rsrc_q, stage + kIvfSlabP + lw * 1024, (cut && qupper) ? kOOB : qvoff, u * kIvfSlabK);
        };
        issue(0);
        if (T > 1) issue(1);
        if (T > 2) issue(2);
        for (int t = 0; t < T; ++t) {
            // this wave's part of slab t has landed; the 9 ops of each newer slab may stay in flight
            if (t + 2 < T)
                asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
            else if (t + 1 < T)
                asm volatile("s_waitcnt vmcnt(9)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            ring_barrier();   // hand-off t: slab t is complete; the consumers have left slab t - 1
            if (t + 3 < T) issue(t + 3);
        }
        return;
    }

    // ==================================== consumers =============================================================
    const int lrow = lane & 31, lhi = lane >> 5;
    i32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    const int swz = (lrow >> 1) & 7;          // (the same for database row 32 wave + lrow and query row lrow)
    const int boff = (wave * 32 + lrow) * 128;
    const int aoff = kIvfSlabP + lrow * 128;

    int cur = 0;
    for (int t = 0; t < T; ++t) {
        ring_barrier();   // hand-off t (see the loaders)
        const char* stage = smem + cur * kIvfStage;
#pragma unroll
        for (int s = 0; s < 4; ++s) {         // k = 128 u + 32 s + 16 lhi + 0..15
            const int ch = (((s * 2 + lhi) ^ swz) << 4);
            const i32x4_t b = *(const i32x4_t*)(stage + boff + ch);
            const i32x4_t a = *(const i32x4_t*)(stage + aoff + ch);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
        }
        cur = cur + 1 == kIvfStages ? 0 : cur + 1;
    }

    // D[i][j]: lane holds database row j = lane & 31 of the strip, group rows i = 8 g + 4 (lane >> 5) + e
    const int r = tile * kIvfRows + wave * 32 + lrow;      // the row's place in its list
    const int n = list_off[l] + r;
    if (n < iend) {
        const float sb = bscales[n];
        const int id = ids[n];
        // the 16 pairs of this lane in three rounds of independent loads (query, column; scale; then the stores)
        int qv[16];
        long cv[16];
        float sq[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int pi = pbase + 8 * (j >> 2) + 4 * lhi + (j & 3);
            const bool ok = pi < p1;
            qv[j] = ok ? pair_q[pi] : -1;
            cv[j] = ok ? (long)pair_col[pi] + r : -1;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((unsigned)qv[j] >= (unsigned)Q || cv[j] >= width) cv[j] = -1;        // a table that does not fit: no store
            sq[j] = cv[j] >= 0 ? qscales[qv[j]] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (cv[j] >= 0) {
                out[(size_t)qv[j] * ldo + cv[j]] = __fmul_rn(__fmul_rn((float)acc[j], sq[j]), sb);
                out_ids[(size_t)qv[j] * ldo + cv[j]] = id;
            }
    }
}

// the scan's admission rules beyond the sizes (c_api.hip reports them): 16-byte pieces, one 2 GB descriptor per operand
bool ivf_scan_i8_admissible(const int8_t* qcodes, int ldq, int Q, const int8_t* bcodes, int ldb) {
    return ((ldq | ldb) & 15) == 0 && ((((uintptr_t)qcodes) | ((uintptr_t)bcodes)) & 15) == 0 &&
           (size_t)ldb * kIvfRows < (1ull << 31) && (size_t)ldq * (size_t)(Q > 0 ? Q : 1) < (1ull << 31);
}

int ivf_scan_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                const float* bscales, const int* ids, int N, int D, const int* list_off, int nlist, const int* pair_off,
                const int* pair_q, const int* pair_col, const int* item_off, int items, float* scores, int* out_ids,
                int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    const long total = (long)Q * width;
    hipLaunchKernelGGL(fill_ids_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out_ids, lds, width, total);
    DIR_HIP_CHECK(hipGetLastError());
    if (items <= 0 || N <= 0) return DIR_OK;
    const int Kp = (D + 63) & ~63, T = ceil_div(Kp, kIvfSlabK);
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_scan_i8_kernel, kIvfLds, attr_done));
    hipLaunchKernelGGL(ivf_scan_i8_kernel, dim3((unsigned)items), dim3(768), kIvfLds, stream, qcodes, ldq, qscales, Q, bcodes,
                       ldb, bscales, ids, N, Kp, T, list_off, nlist, pair_off, pair_q, pair_col, item_off, scores, out_ids,
                       lds, width);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir

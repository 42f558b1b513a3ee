// ivfpq.hip — the IVF-PQ index: residual PQ codes in inverted lists (include/dir_engine.h has the definitions).
//
// The coarse quantiser is ivf.hip's, the encoder and the query tables are pq.hip's; a row's codes are those of its
// residual to the fp32 centroid of its list, so the score of a query against a row of list l is
//     <q, centroid_l>  +  the table entries of the row's codes,
// one chain of fp32 additions that STARTS at the coarse term.  Two kernels are new:
//
// ivfpq_base_kernel - the coarse term of every (query, probed list): one workgroup per slot, thread m runs the chain of
//   sub-space m over its dsub columns, thread 0 adds the M partial sums in order.  Small work.
//
// ivfpq_scan_kernel - the hot path, cut QUERY-major (ivf.hip's int8 scan is list-major because a list's bytes are its
//   expensive operand; here that is the query's table, M KiB in LDS, and a row is M bytes).  A workgroup of 1024 threads
//   owns ONE query and 1024 consecutive columns of that query's concatenated output, one column per thread:
//     1. the slots of the query that meet the workgroup's columns are compacted into LDS (its columns there, their first
//        row, coarse term): every thread looks at nprobe / 1024 slots, a workgroup keeps the few that concern it;
//     2. a thread finds the slot of its column among those, and loads its row's code words into registers (threads of one
//        list are neighbours: their rows are contiguous);
//     3. under those loads the query's table goes to LDS, [sub-space][256] floats as dir_pq_lut wrote it; the sub-spaces
//        past M up to the next multiple of 8 hold -0.0f, the one value with x + v == x in every bit of every x (-0.0f
//        included, which a coarse term can be), so what a code row holds past byte M does not matter;
//     4. the thread adds its row's entries in the order m = 0 .. M - 1, starting from the coarse term of its slot, and
//        stores the score and the row's id.  A column below `width` that no slot covers gets id -1.
//   There is no inverted probe table, no sort and no fill kernel.  1024 look-ups per table entry read: the load of a
//   table (M KiB from L2) stays near an eighth of the LDS time of its look-ups (random 4-byte gathers, about 8 cycles a
//   wave-instruction), while a query of 8 lists of 1000 rows still spreads over 8 workgroups.  Up to M = 64 two workgroups
//   share a CU (64 + 12 KiB of LDS each, 32 waves); above that one (up to 128 + 12 KiB).
//   The kernel comes in five widths (2, 4, 8, 16, 32 code words = M up to 8 .. 128); the words sit in registers and every
//   second word a uniform branch ends the scheduling region, as in pq.hip, so the compiler does not issue every read of a
//   row first and spill the results.  There is no loop over queries here, so the addresses cannot be hoisted out of one.
#include "dir_common.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // coarse terms and scores are defined in single IEEE operations: nothing here may fuse

namespace dir {

// ---- coarse terms ------------------------------------------------------------------------------------------------------
static constexpr int kBaseThreads = 128;  // >= dir_pq_max_m(): one thread per sub-space

__global__ void __launch_bounds__(kBaseThreads) ivfpq_base_kernel(const float* __restrict__ Qm, int ldq,
                                                                  const float* __restrict__ centroids, int ldc, int nlist, int D,
                                                                  int M, const int* __restrict__ probe, int nprobe,
                                                                  float* __restrict__ base) {
    __shared__ __attribute__((aligned(16))) float part[kBaseThreads];
    const int tid = threadIdx.x;
    const long slot = blockIdx.x;
    const int l = probe[slot];                             // uniform
    if ((unsigned)l >= (unsigned)nlist) {
        if (tid == 0) base[slot] = __uint_as_float(0x7fc00000u);
        return;
    }
    const int dsub = D / M;
    const float* q = Qm + (size_t)(slot / nprobe) * ldq + (size_t)tid * dsub;
    const float* c = centroids + (size_t)l * ldc + (size_t)tid * dsub;
    // 16-byte loads where every sub-space starts on one (several in flight per thread; the chain keeps its order)
    const bool vec = ((dsub | ldq | ldc) & 3) == 0 && ((((uintptr_t)Qm) | ((uintptr_t)centroids)) & 15) == 0;
    if (tid < M) {
        float acc = 0.f;
        if (vec) {
#pragma unroll 4
            for (int d = 0; d < dsub; d += 4) {
                const f32x4_t a = *(const f32x4_t*)(q + d), b = *(const f32x4_t*)(c + d);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = acc + a[e] * b[e];
            }
        } else {
#pragma unroll 4
            for (int d = 0; d < dsub; ++d) acc = acc + q[d] * c[d];
        }
        part[tid] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        float acc = 0.f;
        int m = 0;
        for (; m + 4 <= M; m += 4) {
            const f32x4_t s = *(const f32x4_t*)(part + m);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = acc + s[e];
        }
        for (; m < M; ++m) acc = acc + part[m];
        base[slot] = acc;
    }
}

int ivfpq_base(const float* queries, int ldq, int Q, const float* centroids, int ldc, int nlist, int D, int M, const int* probe,
               int nprobe, float* base, hipStream_t stream) {
    const long slots = (long)Q * nprobe;
    if (slots <= 0) return DIR_OK;
    if (M > kBaseThreads) return fail(DIR_ERR_INVALID, "ivfpq_base: M above the sub-spaces of a workgroup");
    if (!launch_fits(slots, kBaseThreads))
        return fail(DIR_ERR_INVALID, "ivfpq_base: Q * nprobe * 128 must stay below 2^32 (one workgroup per slot): cut the queries");
    hipLaunchKernelGGL(ivfpq_base_kernel, dim3((unsigned)slots), dim3(kBaseThreads), 0, stream, queries, ldq, centroids, ldc,
                       nlist, D, M, probe, nprobe, base);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the scan of the probed lists --------------------------------------------------------------------------------------
static constexpr int kScanCols = 1024;    // threads = columns of a workgroup
static constexpr int kScanSlots = 1024;   // slots of at least one row that can meet 1024 columns without overlapping
// per slot: its columns inside the workgroup (first | past-the-last << 16), the row of the first, the coarse term; and their
// count.  12 304 bytes: at M = 64 a workgroup takes 65 536 + 12 304 = 77 840, so two fit the CU's 163 840.
static constexpr int kScanSlotBytes = 3 * 4 * kScanSlots + 16;

int ivfpq_scan_cols() { return kScanCols; }

// Workgroup b: query b / spans, columns (b % spans) * 1024 .. + 1023.  base, probe, col_off: [Q][nprobe], contiguous.
template <int kWords>
__global__ void __launch_bounds__(kScanCols) ivfpq_scan_kernel(const float* __restrict__ lut, int M, const float* __restrict__ base,
                                                               const uint8_t* __restrict__ codes, int ldc,
                                                               const int* __restrict__ ids, int N,
                                                               const int* __restrict__ list_off, int nlist,
                                                               const int* __restrict__ probe, const int* __restrict__ col_off,
                                                               int nprobe, float* __restrict__ scores, int* __restrict__ out_ids,
                                                               int lds, int width, int spans) {
    extern __shared__ __attribute__((aligned(16))) float tab[];
    const int tid = threadIdx.x;
    const int q = (int)(blockIdx.x / (unsigned)spans);
    const int c0 = (int)(blockIdx.x % (unsigned)spans) * kScanCols;
    const int c = c0 + tid;
    const int words = (M + 3) >> 2;
    const int image = min(kWords, (words + 1) & ~1);       // code words whose tables are in LDS: an even number
    // (everything in the dynamic region, the table first: its 16-byte pieces stay aligned)
    uint32_t* s_cols = (uint32_t*)(tab + (size_t)image * 1024);
    int* s_row0 = (int*)(s_cols + kScanSlots);
    float* s_base = (float*)(s_row0 + kScanSlots);
    int& s_count = *(int*)(s_base + kScanSlots);

    // 1. the slots that meet columns c0 .. c0 + 1023 (their order does not matter: at most one covers a column)
    if (tid == 0) s_count = 0;
    __syncthreads();
    for (int p = tid; p < nprobe; p += kScanCols) {
        const size_t sp = (size_t)q * nprobe + p;
        const int l = probe[sp];
        if ((unsigned)l < (unsigned)nlist) {
            const int r0 = list_off[l], r1 = min(list_off[l + 1], N), s = col_off[sp];
            if (r0 >= 0 && r1 > r0 && s < c0 + kScanCols && (long)s + (r1 - r0) > c0) {
                // clipped to the workgroup's columns: lo in [0, 1023], hi in [1, 1024], the row of column c0 + lo in [r0, r1)
                const int lo = max(s, c0) - c0;
                const int hi = (int)(min((long)s + (r1 - r0), (long)c0 + kScanCols) - c0);
                const int i = atomicAdd(&s_count, 1);
                if (i < kScanSlots) {
                    s_cols[i] = (uint32_t)lo | ((uint32_t)hi << 16);
                    s_row0[i] = (int)(r0 + ((long)c0 + lo - s));
                    s_base[i] = base[sp];
                }
            }
        }
    }
    __syncthreads();

    // 2. the row of this thread's column, its codes on their way to registers
    const int count = min(s_count, kScanSlots);
    int row = -1;
    float acc = 0.f;
    if (c < width) {
        // (a linear walk, every read a broadcast: `count` is the slots that meet these 1024 columns - a handful at the list
        // lengths an index is built for.  Every list probed over lists of a row or two makes it up to 1024 steps per thread;
        // sorting the slots for a binary search is the step that case would need)
        for (int i = 0; i < count; ++i) {
            const uint32_t cols = s_cols[i];
            const int lo = (int)(cols & 0xffffu), hi = (int)(cols >> 16);
            if (tid >= lo && tid < hi) row = s_row0[i] + (tid - lo), acc = s_base[i];
        }
    }
    uint32_t code[kWords];
    if (row >= 0) {
        // (a word past M reads the last word: its tables hold -0.0f)
        const uint32_t* src = (const uint32_t*)(codes + (size_t)row * ldc);
#pragma unroll
        for (int w = 0; w < kWords; ++w) code[w] = src[min(w, words - 1)];
    } else {
#pragma unroll
        for (int w = 0; w < kWords; ++w) code[w] = 0u;
    }

    // 3. the table of the query
    {
        const f32x4_t* src = (const f32x4_t*)(lut + (size_t)q * M * 256);
        const f32x4_t kIdentity = {-0.f, -0.f, -0.f, -0.f};
        const int pieces = M * 64, padded = image * 256;   // 16-byte pieces: 64 a sub-space
#pragma unroll 4
        for (int i = tid; i < padded; i += kScanCols) ((f32x4_t*)tab)[i] = i < pieces ? src[i] : kIdentity;
    }
    __syncthreads();

    // 4. the chain, m ascending, from the coarse term
    if (row >= 0) {
#pragma unroll
        for (int w2 = 0; w2 < kWords; w2 += 2) {
            if (w2 < image) {                              // uniform; ends a scheduling region (pq.hip)
#pragma unroll
                for (int w = w2; w < w2 + 2; ++w)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc = acc + tab[(4 * w + b) * 256 + ((code[w] >> (8 * b)) & 255u)];
            }
        }
        scores[(size_t)q * lds + c] = acc;
        out_ids[(size_t)q * lds + c] = ids[row];
    } else if (c < width) {
        out_ids[(size_t)q * lds + c] = -1;
    }
}

template <int kWords>
static int ivfpq_scan_launch(const float* lut, const float* base, int Q, int M, const uint8_t* codes, int ldc, const int* ids,
                             int N, const int* list_off, int nlist, const int* probe, const int* col_off, int nprobe,
                             float* scores, int* out_ids, int lds, int width, hipStream_t stream) {
    const int spans = ceil_div(width, kScanCols);
    const long blocks = (long)Q * spans;
    if (!launch_fits(blocks, kScanCols))
        return fail(DIR_ERR_INVALID, "ivfpq_scan: Q * width (rounded up to 1024 columns) must stay below 2^32: cut the queries");
    const int words = (M + 3) >> 2;
    const int bytes = std::min(kWords, (words + 1) & ~1) * 4096 + kScanSlotBytes;
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivfpq_scan_kernel<kWords>, kWords * 4096 + kScanSlotBytes, attr_done));
    hipLaunchKernelGGL((ivfpq_scan_kernel<kWords>), dim3((unsigned)blocks), dim3(kScanCols), bytes, stream, lut, M, base, codes,
                       ldc, ids, N, list_off, nlist, probe, col_off, nprobe, scores, out_ids, lds, width, spans);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

int ivfpq_scan(const float* lut, const float* base, int Q, int M, const uint8_t* codes, int ldc, const int* ids, int N,
               const int* list_off, int nlist, const int* probe, const int* col_off, int nprobe, float* scores, int* out_ids,
               int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    if (width > (1 << 30)) return fail(DIR_ERR_INVALID, "ivfpq_scan: width above 2^30");
#define DIR_IVFPQ_SCAN(W) \
    ivfpq_scan_launch<W>(lut, base, Q, M, codes, ldc, ids, N, list_off, nlist, probe, col_off, nprobe, scores, out_ids, lds, width, stream)
    if (M <= 8) return DIR_IVFPQ_SCAN(2);
    if (M <= 16) return DIR_IVFPQ_SCAN(4);
    if (M <= 32) return DIR_IVFPQ_SCAN(8);
    if (M <= 64) return DIR_IVFPQ_SCAN(16);
    return DIR_IVFPQ_SCAN(32);
#undef DIR_IVFPQ_SCAN
}

}  // namespace dir

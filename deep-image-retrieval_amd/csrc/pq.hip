// pq.hip — the product-quantised index: encoder, query tables and the table scan (include/dir_engine.h has the definitions).
//
// A row of D floats is cut into M sub-vectors of dsub = D / M values; each is replaced by the number of its nearest of 256
// centroids, so a row is M bytes.  A query is scored through M tables of 256 inner products (asymmetric distance
// computation): score = the sum of one entry per sub-space.  Every number is a chain of single fp32 operations in a fixed
// order, so tests/pq_ref.py reproduces codes, tables and scores bit for bit.
//
// subspace_accumulate - what the encoder and the table kernel share: a workgroup of 256 threads serves ONE sub-space,
//   thread j is centroid j, and a pass accumulates 32 rows at once (32 independent chains per thread: plain VALU work with
//   no dependent-add stalls).  The sub-space's centroids are staged in LDS 32 columns at a time, transposed at a pitch of
//   257 words (thread j reads bank (d + j) % 32: conflict-free); the 32 rows' values of those columns sit beside them and
//   are read as broadcasts.  The chain of a (row, centroid) runs over the columns in order, whatever the staging.
//
// pq_encode_kernel - squared distances by subspace_accumulate, then the arg-min over the 256 threads as the minimum of
//   64-bit keys (distance bits : centroid): distances are >= +0 or NaN, so their bits order as unsigned integers, a NaN maps
//   to the largest key and equal distances fall to the smaller centroid - the scan order of the definition, in any order.
//   A workgroup walks 256 rows of its sub-space and stages a codebook of up to 32 columns once for all of them.
//
// pq_lut_kernel - inner products by subspace_accumulate, 32 queries per workgroup and sub-space.
//
// pq_scan_kernel - the hot path, bound by LDS gathers: 1024 threads (16 waves, the CU's 512 registers per lane shared
//   four ways: 128 each) own a tile of 2048 rows (1024 above M = 64) whose codes sit in registers, two rows (one) per
//   thread; the workgroup walks its queries TWO at a time: the tables of a pair are interleaved entry by entry in LDS, so
//   one 8-byte read serves both, and every thread adds its rows' entries in the order m = 0 .. M - 1.  An image is up to
//   64 sub-spaces of a pair (128 KiB); above M = 64 a pair takes two images, one after the other; up to M = 32 a second
//   image fits and is filled under the look-ups.  A tile reads 256 table entries per sub-space and query and looks 2048
//   (1024) up.  The kernel comes in four widths (M up to 8, 16, 32, 64; above that two phases of 64); an M between two of
//   them runs the wider one on tables of -0.0f.
#include "dir_common.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // codes, tables and scores are defined in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kPqMaxM = 128;       // one query's table, 128 KiB, fits the 160 KiB of LDS
static constexpr int kSubRows = 32;       // rows (queries) of a pass: one accumulator register each
static constexpr int kSubChunk = 32;      // sub-space columns staged at a time
static constexpr int kSubPitch = 257;     // words between two staged columns of the centroids
static constexpr int kSubXPitch = 36;     // ... and of the rows (a multiple of 4: 16-byte broadcast reads)
static constexpr int kEncPasses = 8;      // passes a workgroup of the encoder walks: 256 rows
static constexpr int kEncFold = 16;       // rows whose arg-min is folded at a time (the keys of 32 would pass 64 KiB of LDS)
static constexpr int kLutPasses = 1;

int pq_max_m() { return kPqMaxM; }

// acc[i] <- the chain over the dsub columns of sub-space `col0 / dsub` for row r0 + i (i < rows; the other chains run on
// zeros) against centroid threadIdx.x of cb [256][dsub]: kDist ? acc + (x - c) * (x - c) : acc + x * c.
// cs [kSubChunk * kSubPitch], xs [kSubChunk * kSubXPitch]: LDS.  keep_cb: cs already holds this sub-space's only chunk.
template <bool kDist>
__device__ __forceinline__ void subspace_accumulate(const float* __restrict__ X, int ldx, long r0, int rows,
                                                    const float* __restrict__ cb, int dsub, int col0, float* cs, float* xs,
                                                    bool keep_cb, float (&acc)[kSubRows]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < kSubRows; ++i) acc[i] = 0.f;
    for (int d0 = 0; d0 < dsub; d0 += kSubChunk) {
        const int dc = min(kSubChunk, dsub - d0);
        __syncthreads();                                  // the previous chunk's (pass's) readers are done
        if (!keep_cb) {
            for (int i = tid; i < 256 * dc; i += 256) {
                const int j = i / dc, dd = i - j * dc;
                cs[dd * kSubPitch + j] = cb[(size_t)j * dsub + d0 + dd];
            }
        }
#pragma unroll
        for (int k = 0; k < kSubRows * kSubChunk / 256; ++k) {
            const int i = tid + k * 256, dd = i & (kSubChunk - 1), ri = i >> 5;
            xs[dd * kSubXPitch + ri] = (dd < dc && ri < rows) ? X[(size_t)(r0 + ri) * ldx + col0 + d0 + dd] : 0.f;
        }
        __syncthreads();
        for (int dd = 0; dd < dc; ++dd) {
            const float cv = cs[dd * kSubPitch + tid];
#pragma unroll
            for (int g = 0; g < kSubRows / 4; ++g) {
                const f32x4_t xv = *(const f32x4_t*)(xs + dd * kSubXPitch + 4 * g);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    // (plain operators under the pragma above: the __fmul_rn / __fadd_rn of the HIP headers are inline
                    // functions compiled under the headers' own contraction mode and fuse into an FMA once inlined)
                    if (kDist) {
                        const float t = xv[e] - cv;
                        acc[4 * g + e] = acc[4 * g + e] + t * t;
                    } else {
                        acc[4 * g + e] = acc[4 * g + e] + xv[e] * cv;
                    }
                }
            }
        }
    }
}

// ---- encoder -----------------------------------------------------------------------------------------------------------
// Workgroup b: sub-space b % M, rows (b / M) * 256 .. + 255.
__global__ void __launch_bounds__(256) pq_encode_kernel(const float* __restrict__ X, int ldx, int N, int D, int M,
                                                      const float* __restrict__ codebooks, uint8_t* __restrict__ codes, int ldc) {
    __shared__ __attribute__((aligned(16))) float cs[kSubChunk * kSubPitch];
    __shared__ __attribute__((aligned(16))) float xs[kSubChunk * kSubXPitch];
    __shared__ uint32_t kd[kEncFold * kSubPitch];
    const int tid = threadIdx.x;
    const int m = (int)(blockIdx.x % (unsigned)M);
    const long base = (long)(blockIdx.x / (unsigned)M) * (kEncPasses * kSubRows);
    const int dsub = D / M;
    const float* cb = codebooks + (size_t)m * 256 * dsub;
    const int padM = (M + 3) & ~3;
    float acc[kSubRows];
    for (int p = 0; p < kEncPasses; ++p) {
        const long r0 = base + (long)p * kSubRows;
        if (r0 >= N) break;                                // uniform
        const int rows = (int)min((long)kSubRows, (long)N - r0);
        subspace_accumulate<true>(X, ldx, r0, rows, cb, dsub, m * dsub, cs, xs, p > 0 && dsub <= kSubChunk, acc);
        // the arg-min, 16 rows at a time: 16 threads per row, thread s of them scans the centroids s, s + 16, ... in
        // ascending order, then the 16 (key, centroid) pairs fold to their minimum
#pragma unroll
        for (int h = 0; h < kSubRows / kEncFold; ++h) {
            if (h) __syncthreads();                        // the scan of the previous 16 rows is done
#pragma unroll
            for (int i = 0; i < kEncFold; ++i) {
                const float d = acc[h * kEncFold + i];
                kd[i * kSubPitch + tid] = d != d ? 0xffffffffu : __float_as_uint(d);     // (bank (i + tid) % 32)
            }
            __syncthreads();
            const int ri = tid >> 4, s = tid & 15;
            uint32_t bk = kd[ri * kSubPitch + s], bj = (uint32_t)s;
#pragma unroll
            for (int jj = 1; jj < 16; ++jj) {
                const uint32_t j = (uint32_t)(s + 16 * jj), k = kd[ri * kSubPitch + j];
                if (k < bk) bk = k, bj = j;
            }
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) {
                const uint32_t ok = (uint32_t)__shfl_xor((int)bk, sh), oj = (uint32_t)__shfl_xor((int)bj, sh);
                if (ok < bk || (ok == bk && oj < bj)) bk = ok, bj = oj;
            }
            const int rr = h * kEncFold + ri;
            if (s == 0 && rr < rows) {
                uint8_t* row = codes + (size_t)(r0 + rr) * ldc;
                row[m] = (uint8_t)bj;
                if (m == M - 1)
                    for (int c = M; c < padM; ++c) row[c] = 0;
            }
        }
    }
}

int pq_encode(const float* X, int ldx, int N, int D, int M, const float* codebooks, uint8_t* codes, int ldc, hipStream_t stream) {
    if (N <= 0) return DIR_OK;
    const long blocks = (long)ceil_div(N, kEncPasses * kSubRows) * M;
    if (!launch_fits(blocks, 256))
        return fail(DIR_ERR_INVALID, "pq_encode: N * M (N rounded up to 256 rows) must stay below 2^32: cut the rows");
    hipLaunchKernelGGL(pq_encode_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, X, ldx, N, D, M, codebooks, codes, ldc);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- query tables ------------------------------------------------------------------------------------------------------
// Workgroup b: sub-space b % M, queries (b / M) * 32 .. + 31.
__global__ void __launch_bounds__(256) pq_lut_kernel(const float* __restrict__ Qm, int ldq, int Q, int D, int M,
                                                   const float* __restrict__ codebooks, float* __restrict__ lut) {
    __shared__ __attribute__((aligned(16))) float cs[kSubChunk * kSubPitch];
    __shared__ __attribute__((aligned(16))) float xs[kSubChunk * kSubXPitch];
    const int tid = threadIdx.x;
    const int m = (int)(blockIdx.x % (unsigned)M);
    const long base = (long)(blockIdx.x / (unsigned)M) * (kLutPasses * kSubRows);
    const int dsub = D / M;
    const float* cb = codebooks + (size_t)m * 256 * dsub;
    float acc[kSubRows];
    for (int p = 0; p < kLutPasses; ++p) {
        const long r0 = base + (long)p * kSubRows;
        if (r0 >= Q) break;
        const int rows = (int)min((long)kSubRows, (long)Q - r0);
        subspace_accumulate<false>(Qm, ldq, r0, rows, cb, dsub, m * dsub, cs, xs, p > 0 && dsub <= kSubChunk, acc);
#pragma unroll
        for (int i = 0; i < kSubRows; ++i)
            if (i < rows) lut[((size_t)(r0 + i) * M + m) * 256 + tid] = acc[i];
    }
}

int pq_lut(const float* queries, int ldq, int Q, int D, int M, const float* codebooks, float* lut, hipStream_t stream) {
    if (Q <= 0) return DIR_OK;
    const long blocks = (long)ceil_div(Q, kLutPasses * kSubRows) * M;
    if (!launch_fits(blocks, 256))
        return fail(DIR_ERR_INVALID, "pq_lut: Q * M * 8 (Q rounded up to 32 queries) must stay below 2^32: cut the queries");
    hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, queries, ldq, Q, D, M, codebooks, lut);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
static constexpr int kScanThreads = 1024;
static constexpr int kScanMinQueries = 8;   // queries a workgroup takes at least (all of them when there are fewer): its codes are read once

// kWords: code words (4 sub-spaces each) of an LDS image, kPhases: images per row (a row holds kWords * kPhases words in
// registers), kRows: rows per thread.
// Workgroup (x, y): rows x * 1024 * kRows .. (row r of thread t is + r * 1024 + t: the score stores of a wave are
// contiguous), queries y * qper .. + qper - 1, taken TWO at a time: an image is [4 * kWords][256][2] floats - the tables of
// 4 * kWords sub-spaces for both queries, interleaved entry by entry, so ONE ds_read_b64 fetches the entries of both (a
// gather of 8-byte entries meets the bank conflicts of a gather of 4-byte ones and carries twice the data).  A step is a
// pair of queries; above M = 64 it has two phases, sub-spaces 0 .. 63 and 64 .. 127, whose images follow each other
// through the same 128 KiB while the chains stay in their registers.  two: a second image fits (128 KiB in all) and is
// filled while the first is read; else the next image waits in registers over the look-ups and is written between two
// barriers.
//
// An image has 4 * kWords sub-spaces whatever M is: the tables past M hold -0.0f, the one value x + v == x holds for in
// every bit of every x a chain can reach (the chain starts at +0.0f, so it is never -0.0f).  What a code row holds in the
// bytes past M does not matter.
//
// The index of a look-up is a byte of a code word, a value that does not change from step to step: left alone, the
// compiler computes every LDS address once, ahead of the loop, and spills them.  The words are therefore rotated by one
// byte per step (in step s sub-space 4 w + b sits at byte (b + s + 1) % 4), which keeps the extraction - a shift by a
// uniform amount and a mask - inside the loop.
template <int kWords, int kPhases, int kRows>
__global__ void __launch_bounds__(kScanThreads) pq_scan_kernel(const float* __restrict__ lut, int Q, int M,
                                                             const uint8_t* __restrict__ codes, int ldc, int N,
                                                             float* __restrict__ scores, int lds, int qper, int two) {
    extern __shared__ __attribute__((aligned(16))) float tab[];
    constexpr int kPieces = kWords * 4 * 64;               // 16-byte pieces of one query's part of an image
    constexpr int kFetch = (kPieces + kScanThreads - 1) / kScanThreads;
    constexpr size_t image = (size_t)2 * kPieces * 4;      // floats
    const int tid = threadIdx.x;
    const long tile0 = (long)blockIdx.x * (kScanThreads * kRows);
    const int q0 = blockIdx.y * qper, q1 = min(Q, q0 + qper);
    const int words = (M + 3) >> 2, pieces = M * 64;
    const int steps = (q1 - q0 + 1) / 2;
    const f32x4_t kIdentity = {-0.f, -0.f, -0.f, -0.f};

    uint32_t code[kRows][kWords * kPhases];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const long row = tile0 + (long)r * kScanThreads + tid;
        // (every load unconditional, so that they are all in flight at once: a row past N reads the last row and stores
        // nothing, a word past M reads the last word and is never looked up)
        const uint32_t* src = (const uint32_t*)(codes + (size_t)(row < N ? row : N - 1) * ldc);
#pragma unroll
        for (int w = 0; w < kWords * kPhases; ++w) code[r][w] = src[min(w, words - 1)];
    }
    // (the first rotation, here: a use of every word ahead of the loop, so no look-up waits for the loads of this block)
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
        for (int w = 0; w < kWords * kPhases; ++w) code[r][w] = __builtin_rotateleft32(code[r][w], 8);

    f32x4_t pf[2][kFetch];
    auto fetch = [&](int step, int phase) __attribute__((always_inline)) {
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int q = q0 + step * 2 + g;               // (a last, single query runs beside a copy of the first)
            const f32x4_t* src = (const f32x4_t*)(lut + (size_t)(q < q1 ? q : q0) * M * 256);
#pragma unroll
            for (int k = 0; k < kFetch; ++k) {
                const int i = phase * kPieces + tid + k * kScanThreads;
                pf[g][k] = i < pieces ? src[i] : kIdentity;
            }
        }
    };
    auto put = [&](float* dst) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < kFetch; ++k) {
            const int i = tid + k * kScanThreads;
            if (i < kPieces) {                             // entries 4 i .. 4 i + 3 of both tables, interleaved
                ((f32x4_t*)dst)[2 * i] = f32x4_t{pf[0][k][0], pf[1][k][0], pf[0][k][1], pf[1][k][1]};
                ((f32x4_t*)dst)[2 * i + 1] = f32x4_t{pf[0][k][2], pf[1][k][2], pf[0][k][3], pf[1][k][3]};
            }
        }
    };
    // the two chains of a row as ONE vector add per look-up - each lane of it a single IEEE add - written as such, so that
    // no vectoriser collects the scalar adds of a step behind its last read
    f32x2_t acc[kRows];
    auto look_up = [&](const float* t, int step, int phase) __attribute__((always_inline)) {
        uint32_t shift[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) shift[b] = 8u * ((uint32_t)(b + step + 1) & 3u);
        const f32x2_t* te = (const f32x2_t*)t;
#pragma unroll
        for (int w2 = 0; w2 < kWords; w2 += 2) {
            // (a uniform branch per two words: it skips the words an M below the kernel's width does not have, and - its
            // purpose - it ends a scheduling region: over one straight-line step the compiler issues every read first and
            // spills the results)
            if (phase * kWords + w2 < words) {
#pragma unroll
                for (int w = w2; w < w2 + 2; ++w)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int r = 0; r < kRows; ++r)
                            acc[r] = acc[r] + te[(4 * w + b) * 256 + ((code[r][phase * kWords + w] >> shift[b]) & 255u)];
            }
        }
    };

    if (steps <= 0) return;
    fetch(0, 0);
    put(tab);
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < steps; ++step) {
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = f32x2_t{0.f, 0.f};
#pragma unroll
        for (int phase = 0; phase < kPhases; ++phase) {
            const int stage = step * kPhases + phase;
            const bool more = phase + 1 < kPhases || step + 1 < steps;             // uniform
            if (more) fetch(phase + 1 < kPhases ? step : step + 1, phase + 1 < kPhases ? phase + 1 : 0);
            look_up(two ? tab + (size_t)(stage & 1) * image : tab, step, phase);
            if (more) {
                if (!two) __syncthreads();                 // every look-up of this image is done
                put(two ? tab + (size_t)((stage + 1) & 1) * image : tab);   // (two: last read before the barrier that ended stage - 1)
            }
            __syncthreads();
        }
        const int q = q0 + step * 2;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const long row = tile0 + (long)r * kScanThreads + tid;
            if (row < N) {
                scores[(size_t)q * lds + row] = acc[r][0];
                if (q + 1 < q1) scores[(size_t)(q + 1) * lds + row] = acc[r][1];
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int w = 0; w < kWords * kPhases; ++w) code[r][w] = __builtin_rotateleft32(code[r][w], 8);
    }
}

template <int kWords, int kPhases, int kRows>
static int pq_scan_launch(const float* lut, int Q, int M, const uint8_t* codes, int ldc, int N, float* scores, int lds,
                          hipStream_t stream) {
    const int tiles = ceil_div(N, kScanThreads * kRows);
    // enough workgroups for four rounds of the CUs: the queries are cut where the rows alone give too few
    const int split = min(Q, max(1, ceil_div(4 * cu_count(), tiles)));
    const int qper = max(max(ceil_div(Q, split), min(Q, kScanMinQueries)), ceil_div(Q, 65535));
    constexpr int image = 2 * kWords * 4096, two = 2 * image <= 128 * 1024;
    static_assert(image <= 128 * 1024, "one image must fit LDS");
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)pq_scan_kernel<kWords, kPhases, kRows>, (two ? 2 : 1) * image, attr_done));
    hipLaunchKernelGGL((pq_scan_kernel<kWords, kPhases, kRows>), dim3((unsigned)tiles, (unsigned)ceil_div(Q, qper)),
                       dim3(kScanThreads), (two ? 2 : 1) * image, stream, lut, Q, M, codes, ldc, N, scores, lds, qper, (int)two);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

int pq_scan(const float* lut, int Q, int M, const uint8_t* codes, int ldc, int N, float* scores, int lds, hipStream_t stream) {
    if (Q <= 0 || N <= 0) return DIR_OK;
    if (M <= 8) return pq_scan_launch<2, 1, 2>(lut, Q, M, codes, ldc, N, scores, lds, stream);
    if (M <= 16) return pq_scan_launch<4, 1, 2>(lut, Q, M, codes, ldc, N, scores, lds, stream);
    if (M <= 32) return pq_scan_launch<8, 1, 2>(lut, Q, M, codes, ldc, N, scores, lds, stream);
    if (M <= 64) return pq_scan_launch<16, 1, 2>(lut, Q, M, codes, ldc, N, scores, lds, stream);
    return pq_scan_launch<16, 2, 1>(lut, Q, M, codes, ldc, N, scores, lds, stream);
}

}  // namespace dir

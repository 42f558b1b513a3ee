// cov_f32.hip — the N-dependent half of a PCA fit on the matrix cores (v_mfma_f32_32x32x2_f32), gfx950.
//
//   a[n][i]  = X[n][i] - shift[i]                       fp32, subtracted at load, before any product
//   gram[i][j] += sum_n a[n][i] * a[n][j]               fp64 [D][D], both triangles, bit-symmetric
//   sums[i]    += sum_n a[n][i]                         fp64 [D]
//
// A symmetric "TN" Gram product: it contracts over the ROWS of X (gemm_f32.hip's NT form contracts over the contiguous
// dimension).  There is no reference code for the fit - the reference only ships the Landmarks18_pca image list - the
// result is what dirtorch/utils/common.py:221-232 reads back (mean_, components_, explained_variance_ of the PCA that
// dirtorch_amd/whitening.py derives from gram and sums on the host).
//
// Arithmetic.  The shifted-data form: with shift close to the column mean the later sums sums^T / n correction is tiny
// and nothing cancels (L2-normalised descriptors have a strong common mean; X^T X - n m m^T on raw data would lose it).
// The f32 MFMA is bit-for-bit an n-ordered fmaf chain with exact products; a chain runs over at most kCovChainRows rows
// and is then folded into an fp64 accumulator in registers, so the error of an entry is bounded by
// (kCovChainRows + 3) 2^-24 sum_n |a_ni| |a_nj| however many rows the call has.
//
// Launch shape.  Upper-triangle tiles of 128 x 128 (136 of 256 at D = 2048) x row slices (blockIdx.y), so that all CUs
// have work; the tiles of a slice are dispatched together and walk the rows in step, so an X slab comes from HBM once
// and from L2 for the tiles that share it.  Every (tile, slice) workgroup writes its fp64 tile to stream-ordered
// scratch; cov_reduce_kernel adds the slices in slice order into gram - the upper entry and its mirror receive the same
// value - and the column sums (a ones fragment on the diagonal tiles: the same chains, the same folds) into sums.
// No floating-point atomics: two calls on the same input give the same bits.
#include "dir_common.h"
#include "pointwise.h"

namespace dir {

#ifndef DIR_COV_CHAIN_ROWS           // (experiment builds: -DDIR_COV_CHAIN_ROWS=n is how the cost of R was measured)
#define DIR_COV_CHAIN_ROWS 128
#endif
constexpr int kCovChainRows = DIR_COV_CHAIN_ROWS;   // R: rows one fp32 chain runs over before it is folded into fp64
constexpr int kCovSlab = 32;                        // rows of X per LDS stage
static_assert(kCovChainRows >= kCovSlab && kCovChainRows % kCovSlab == 0, "R must be a multiple of the slab");
constexpr int kCovTile = 128;        // columns per tile side
constexpr int kCovMaxSlices = 64;
constexpr int kCovMinSliceRows = 4 * kCovChainRows;
constexpr int kCovTargetBlocks = 512;   // two rounds of workgroups on 256 CUs

int cov_chain_rows() { return kCovChainRows; }

// tile index -> (ti, tj), ti <= tj, row-major over the upper triangle of T x T tiles
__device__ inline void cov_tile_of(int tile, int T, int& ti, int& tj) {
    int i = 0, rem = tile;
    while (rem >= T - i) {
        rem -= T - i;
        ++i;
    }
    ti = i;
    tj = i + rem;
}

// One (tile, slice) workgroup.  VEC: 16-byte loads (D, ldx multiples of 4, 16-byte aligned bases); DIAG: ti == tj - one panel
// serves both operands and the column sums ride along on a ones fragment.  Both are compile-time so that the K loop is
// straight-line code: the loads of slab s + 1 are issued before the MFMAs of slab s and waited for after them, and the
// fragment reads of a k-step are in flight during the MFMAs of the one before.
template <bool VEC, bool DIAG>
__device__ __forceinline__ void cov_tile(char* smem, const float* __restrict__ X, size_t ldx, int N, int D,
                                         const float* __restrict__ shift, int T, int ti, int tj, int slice_rows,
                                         double* __restrict__ ptile, double* __restrict__ psums) {
    constexpr int SLAB_BYTES = kCovSlab * kCovTile * 4;   // 16 KiB: 32 rows x 128 floats, row-major as in X
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = ti * kCovTile, j0 = tj * kCovTile;
    const int n_begin = (int)blockIdx.y * slice_rows;
    const int n_end = min(N, n_begin + slice_rows);   // (n_begin < N: the host launches no empty slice)

    // staging: thread -> 4 floats of column c4 * 4 in rows r0 + 8 q of the slab; the column is fixed, so is its shift
    const int c4 = tid & 31, r0 = tid >> 5;
    const int coli = i0 + c4 * 4, colj = j0 + c4 * 4;
    f32x4_t shi = {0.f, 0.f, 0.f, 0.f}, shj = shi;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (coli + e < D) shi[e] = shift[coli + e];
        if (!DIAG && colj + e < D) shj[e] = shift[colj + e];
    }
    // VEC: every load is issued, from an address clamped into the matrix; what lies outside is masked at commit
    const int ci = VEC ? min(coli, D - 4) : coli, cj = VEC ? min(colj, D - 4) : colj;
    f32x4_t ri[4], rj[4];
    int rows_ok = 0;   // bit q: row r0 + 8 q of the fetched slab lies inside the slice
    auto fetch = [&](int n0) {
        rows_ok = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int n = n0 + r0 + 8 * q;
            const bool rok = n < n_end;
            rows_ok |= (int)rok << q;
            if constexpr (VEC) {
                const float* row = X + (size_t)min(n, N - 1) * ldx;
                ri[q] = *(const DIR_GLOBAL f32x4_t*)(row + ci);
                if (!DIAG) rj[q] = *(const DIR_GLOBAL f32x4_t*)(row + cj);
            } else {   // any D, pitch and alignment: element by element
                const float* row = X + (size_t)n * ldx;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ri[q][e] = rok && coli + e < D ? row[coli + e] : 0.f;
                    if (!DIAG) rj[q][e] = rok && colj + e < D ? row[colj + e] : 0.f;
                }
            }
        }
    };
    // a = X - shift in fp32, here, before any product; zero padding (rows past the slice, columns past D) stays zero:
    // 0 - shift would leak the shift in
    auto commit = [&](char* stage) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool rok = (rows_ok >> q) & 1;
            f32x4_t v, u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = rok && coli + e < D ? ri[q][e] - shi[e] : 0.f;
                if (!DIAG) u[e] = rok && colj + e < D ? rj[q][e] - shj[e] : 0.f;
            }
            *(f32x4_t*)(stage + (r0 + 8 * q) * 512 + c4 * 16) = v;
            if (!DIAG) *(f32x4_t*)(stage + SLAB_BYTES + (r0 + 8 * q) * 512 + c4 * 16) = u;
        }
    };

    // MFMA operands: lane l holds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; here k is a row of the slab
    // and both operands are read along it: 32 consecutive floats per half-wave, conflict-free ds_read_b32
    const int lrow = lane & 31, lhi = lane >> 5;
    const int aoff = lhi * 512 + (wave * 32 + lrow) * 4;
    const int boff = (DIAG ? 0 : SLAB_BYTES) + lhi * 512 + lrow * 4;

    f32x16_t acc[4], accs;
    double acc64[4][16], accs64[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            acc[t][e] = 0.f;
            acc64[t][e] = 0.0;
        }
        accs[e] = 0.f;
        accs64[e] = 0.0;
    }
    auto compute = [&](const char* stage) {
        float af = *(const float*)(stage + aoff), bf[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bf[t] = *(const float*)(stage + boff + t * 128);
#pragma unroll
        for (int ks = 0; ks < kCovSlab / 2; ++ks) {
            float an = 0.f, bn[4] = {0.f, 0.f, 0.f, 0.f};
            if (ks + 1 < kCovSlab / 2) {
                an = *(const float*)(stage + aoff + (ks + 1) * 1024);
#pragma unroll
                for (int t = 0; t < 4; ++t) bn[t] = *(const float*)(stage + boff + (ks + 1) * 1024 + t * 128);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af, bf[t], acc[t], 0, 0, 0);
            if (DIAG) accs = __builtin_amdgcn_mfma_f32_32x32x2f32(af, 1.0f, accs, 0, 0, 0);
            af = an;
#pragma unroll
            for (int t = 0; t < 4; ++t) bf[t] = bn[t];
        }
    };
    auto fold = [&]() {   // the end of an fp32 chain: into fp64 (the conversion is exact), start the next chain at zero
#pragma unroll
        for (int e = 0; e < 16; ++e) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc64[t][e] += (double)acc[t][e];
                acc[t][e] = 0.f;
            }
            if (DIAG) {
                accs64[e] += (double)accs[e];
                accs[e] = 0.f;
            }
        }
    };

    const int S = (n_end - n_begin + kCovSlab - 1) / kCovSlab;
    char* stage0 = smem;
    char* stage1 = smem + 2 * SLAB_BYTES;
    fetch(n_begin);
    commit(stage0);
    __syncthreads();
    for (int s = 0; s < S; ++s) {
        char* cur = (s & 1) ? stage1 : stage0;
        char* nxt = (s & 1) ? stage0 : stage1;
        fetch(n_begin + (s + 1) * kCovSlab);   // (past the slice: masked, from clamped addresses)
        // (the scheduler otherwise sinks the loads below the MFMAs, next to the commit that waits for them: with one wave
        // per SIMD nothing else hides their latency)
        __builtin_amdgcn_sched_barrier(0);
        compute(cur);
        if ((s + 1) % (kCovChainRows / kCovSlab) == 0) fold();
        commit(nxt);
        __syncthreads();
    }
    fold();

    // D[i][j]: lane holds column j = lane & 31, rows i = 8 g + 4 (lane >> 5) + 0..3; the whole 128 x 128 tile is written
    // (padding rows / columns are exact zeros), cov_reduce_kernel picks what lies inside D x D
    const int tiles = T * (T + 1) / 2;
    double* pt = ptile + ((size_t)blockIdx.y * tiles + blockIdx.x) * (size_t)(kCovTile * kCovTile);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                pt[(wave * 32 + 8 * g + 4 * lhi + e) * kCovTile + t * 32 + lrow] = acc64[t][4 * g + e];
    if (DIAG && lrow == 0) {   // every column of the ones product holds the same sums: column 0's lanes store them
        double* ps = psums + ((size_t)blockIdx.y * T + ti) * kCovTile;
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) ps[wave * 32 + 8 * g + 4 * lhi + e] = accs64[4 * g + e];
    }
}

template <bool VEC>
__global__ void __launch_bounds__(256) cov_gram_kernel(const float* __restrict__ X, size_t ldx, int N, int D,
                                                      const float* __restrict__ shift, int T, int slice_rows,
                                                      double* __restrict__ ptile, double* __restrict__ psums) {
    __shared__ __attribute__((aligned(16))) char smem[4 * kCovSlab * kCovTile * 4];   // two stages x (i panel, j panel)
    int ti, tj;
    cov_tile_of((int)blockIdx.x, T, ti, tj);
    if (ti == tj)
        cov_tile<VEC, true>(smem, X, ldx, N, D, shift, T, ti, tj, slice_rows, ptile, psums);
    else
        cov_tile<VEC, false>(smem, X, ldx, N, D, shift, T, ti, tj, slice_rows, ptile, psums);
}

// gram / sums += the slices' partials, added in slice order (run-to-run identical).  blockIdx.x < tiles * 64: 256 entries
// of an upper tile each - entry (i, j), i <= j, and its mirror receive the same value; the blocks after them: the sums.
__global__ void __launch_bounds__(256) cov_reduce_kernel(const double* __restrict__ ptile,
                                                        const double* __restrict__ psums, int D, int T, int slices,
                                                        double* __restrict__ gram, double* __restrict__ sums) {
    constexpr int TT = kCovTile * kCovTile;
    const int tiles = T * (T + 1) / 2;
    const int b = (int)blockIdx.x;
    if (b >= tiles * (TT / 256)) {
        const int i = (b - tiles * (TT / 256)) * 256 + (int)threadIdx.x;
        if (i >= D) return;
        double r = 0.0;
        for (int z = 0; z < slices; ++z) r += psums[(size_t)z * T * kCovTile + i];
        sums[i] += r;
        return;
    }
    const int tile = b / (TT / 256);
    int ti, tj;
    cov_tile_of(tile, T, ti, tj);
    const int idx = (b % (TT / 256)) * 256 + (int)threadIdx.x;
    const int i = ti * kCovTile + idx / kCovTile, j = tj * kCovTile + idx % kCovTile;
    if (i >= D || j >= D || i > j) return;
    double r = 0.0;
    for (int z = 0; z < slices; ++z) r += ptile[((size_t)z * tiles + tile) * TT + idx];
    gram[(size_t)i * D + j] += r;
    if (i != j) gram[(size_t)j * D + i] += r;
}

int cov_accumulate(const float* X, int ldx, int N, int D, const float* shift, double* gram, double* sums,
                   hipStream_t stream) {
    if (N < 0 || D < 1) return fail(DIR_ERR_INVALID, "cov_accumulate: N must be >= 0 and D >= 1");
    if (ldx < D) return fail(DIR_ERR_INVALID, "cov_accumulate: ldx < D");
    if ((!X && N > 0) || !shift || !gram || !sums) return fail(DIR_ERR_INVALID, "cov_accumulate: null pointer");   // (an empty X has no address)
    if (((uintptr_t)X & 3) || ((uintptr_t)shift & 3) || ((uintptr_t)gram & 7) || ((uintptr_t)sums & 7))
        return fail(DIR_ERR_INVALID, "cov_accumulate: X, shift must be 4-byte and gram, sums 8-byte aligned");
    if (N == 0) return DIR_OK;
    const int T = ceil_div(D, kCovTile);
    const long tiles = (long)T * (T + 1) / 2;
    if (tiles > 65535) return fail(DIR_ERR_INVALID, "cov_accumulate: D too large");
    // row slices: enough workgroups for two rounds of the chip, every slice at least a few chains long
    long want = (kCovTargetBlocks + tiles - 1) / tiles;
    if (want > kCovMaxSlices) want = kCovMaxSlices;
    const long fit = ((long)N + kCovMinSliceRows - 1) / kCovMinSliceRows;
    if (want > fit) want = fit;
    if (want < 1) want = 1;
    int slice_rows = (int)((((long)N + want - 1) / want + kCovSlab - 1) / kCovSlab) * kCovSlab;
    const int slices = (int)(((long)N + slice_rows - 1) / slice_rows);   // (rounding up the slice may leave fewer of them)
    const bool vec_ok = !(D & 3) && !(ldx & 3) && !((uintptr_t)X & 15) && !((uintptr_t)shift & 15);
    const size_t tile_elems = (size_t)slices * tiles * kCovTile * kCovTile;
    const size_t sum_elems = (size_t)slices * T * kCovTile;
    double* scratch = nullptr;
    if (hipMallocAsync((void**)&scratch, (tile_elems + sum_elems) * sizeof(double), stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DIR_ERR_NOMEM, "cov_accumulate: no stream-ordered scratch for the slice partials");
    }
    const dim3 grid((unsigned)tiles, (unsigned)slices);
    if (vec_ok)
        hipLaunchKernelGGL(cov_gram_kernel<true>, grid, dim3(256), 0, stream, X, (size_t)ldx, N, D, shift, T, slice_rows,
                           scratch, scratch + tile_elems);
    else
        hipLaunchKernelGGL(cov_gram_kernel<false>, grid, dim3(256), 0, stream, X, (size_t)ldx, N, D, shift, T, slice_rows,
                           scratch, scratch + tile_elems);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        const unsigned blocks = (unsigned)(tiles * (kCovTile * kCovTile / 256) + ceil_div(D, 256));
        hipLaunchKernelGGL(cov_reduce_kernel, dim3(blocks), dim3(256), 0, stream, scratch, scratch + tile_elems, D, T,
                           slices, gram, sums);
        e = hipGetLastError();
    }
    const hipError_t fe = hipFreeAsync(scratch, stream);
    if (e == hipSuccess) e = fe;
    DIR_HIP_CHECK(e);
    return DIR_OK;
}

}  // namespace dir

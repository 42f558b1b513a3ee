// flat_scan.h — what the flat code scans (index_i8.hip, index_fp4.hip, index_bin.hip) share, once: the frame of a scan
// workgroup, the epilogue that scales and stores a block of scores, and the two launchers of the host side.
//
// A flat scan is strip_stream.h's pipeline over the whole database: workgroup (x, y) takes the 256 rows of tile x against
// the 96 queries of block y.  Its loader waves (8 .. 11) read the tile through one descriptor based at the tile's rows and
// the block's query image through another; consumer wave w owns rows 32 w .. 32 w + 31 of the tile.  A score is
//     out[q][n] = (num * qscales[q]) * bscales[n]
// in two single fp32 multiplications, num the kernel's exact numerator.
//
// What a kernel adds: its stage geometry and the body of its loader and consumer waves, the numerator of a score.
//
// NOT here: the two-pass row walk of the three row quantisers.  Two shared forms were tried (the lane's eight quads as a
// member of a walk struct; as an array of the kernel handed to both passes); hipcc gave 57 / 62 / 69 and 84 / 124 / 124
// VGPRs where the three kernels as written have 90 / 69 / 73, each form moving kernels across an occupancy step and the
// first costing the int8 quantiser 1.2 % (profiles/flat_scan_refactor.txt).  The kernels keep their own copies of the
// walk; they share their launcher.
#pragma once
#include "strip_stream.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

// ---- the frame ---------------------------------------------------------------------------------------------------------
// Every field is workgroup-uniform.
struct FlatFrame {
    int tile, qb;            // the tile of 256 rows (grid x) and the block of 96 queries (grid y)
    int i0, rows, NP;        // the tile's first row, how many rows it has, the rows of the database

    __device__ __forceinline__ FlatFrame(int NP_)
        : tile(blockIdx.x), qb(blockIdx.y), i0(tile * kStripRows), rows(min(kStripRows, NP_ - i0)), NP(NP_) {}
    // one descriptor per workgroup, based at its rows: Kb bytes of every row (of pitch ldp) are readable
    template <class T>
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t database(const T* P, int ldp, int Kb) const {
        return buffer_rsrc(P + (size_t)i0 * ldp, (uint32_t)(((size_t)rows - 1) * ldp + Kb));
    }
    // the query image of this block: `slabs` images of `bytes` each, the blocks one after the other
    template <class T>
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t image(const T* img, int slabs, int bytes) const {
        return buffer_rsrc(img + (size_t)qb * slabs * bytes, (uint32_t)(slabs * bytes));
    }
    // the database row of a consumer lane (stored only where n < NP)
    __device__ __forceinline__ int n(int wave, const StripLane& L) const { return i0 + wave * 32 + L.lrow; }
};

// ---- the epilogue ------------------------------------------------------------------------------------------------------
// Accumulator element 4 g + e of block j of a consumer lane is (query qb * 96 + L.qrow(j, g) + e, the lane's database row
// n).  num(j, 4 g + e, q) is its numerator as a float; it is called for q < NQ only, so it may read what the query has.
template <class Num>
__device__ __forceinline__ void flat_store(const FlatFrame& f, const StripLane& L, int n, const float* __restrict__ qscales,
                                           const float* __restrict__ bscales, float* __restrict__ out, int ldo, int NQ,
                                           Num&& num) {
    if (n >= f.NP) return;
    const float sb = bscales[n];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = f.qb * kQB + L.qrow(j, g) + e;
                if (q < NQ) out[(size_t)q * ldo + n] = __fmul_rn(__fmul_rn(num(j, 4 * g + e, q), qscales[q]), sb);
            }
}

// ---- the host side ---------------------------------------------------------------------------------------------------
// Templates, so that a launcher's callables are plain lambdas of the file that defines the kernel: every hipLaunchKernelGGL
// stays there by name, and a call allocates nothing.

// The launch of a one-wave-per-row kernel over `rows` rows (the three row quantisers; index_bin.hip's code_sums): four rows
// per workgroup, the extent refused under the entry's name `who`, `size` being the entry's name of the row count.
template <class Launch>
int rows_launch(const char* who, const char* size, int rows, Launch&& launch) {
    if (rows <= 0) return DIR_OK;
    const long blocks = ((long)rows + 3) / 4;
    if (!launch_fits(blocks, 256))
        return fail(DIR_ERR_INVALID, std::string(who) + ": " + size + " * 64 must stay below 2^32 (one wave per row): cut the rows");
    launch((unsigned)blocks);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

// The launch of a flat scan of Q queries against N rows, under the entry's name `who`: the empty call, the two launch-extent
// refusals, the kernel's dynamic LDS, `scratch_bytes` of stream-ordered scratch for prepare(scratch) -> hipError_t - the
// kernels that make what the scan reads there - and scan(scratch, grid), the launch of `kernel` itself; the scratch is
// freed behind them.
template <class Prepare, class Scan>
int flat_scan_launch(const char* who, int Q, int N, size_t scratch_bytes, const void* kernel, int lds_bytes,
                     std::atomic<uint64_t>& attr_done, hipStream_t stream, Prepare&& prepare, Scan&& scan) {
    if (Q <= 0 || N <= 0) return DIR_OK;
    const int qblocks = ceil_div(Q, kQB);
    if (qblocks > kMaxGridYZ) return fail(DIR_ERR_INVALID, std::string(who) + ": more than 65535 * 96 queries in one call");
    if (!launch_fits(ceil_div(N, kStripRows), 768))
        return fail(DIR_ERR_INVALID, std::string(who) + ": N * 3 must stay below 2^32 (768 threads per 256 rows): cut the database");
    DIR_HIP_CHECK(ensure_dynamic_lds(kernel, lds_bytes, attr_done));
    char* scratch = nullptr;
    if (hipMallocAsync((void**)&scratch, scratch_bytes, stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(DIR_ERR_NOMEM, std::string(who) + ": no stream-ordered scratch for the query image");
    }
    hipError_t e = prepare(scratch);
    if (e == hipSuccess) {
        scan(scratch, dim3(ceil_div(N, kStripRows), qblocks));
        e = hipGetLastError();
    }
    const hipError_t fe = hipFreeAsync(scratch, stream);
    if (e == hipSuccess) e = fe;
    DIR_HIP_CHECK(e);
    return DIR_OK;
}

}  // namespace dir

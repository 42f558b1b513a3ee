// ivf_scan.h — what the list-major scans of the inverted files (ivf.hip, ivf_fp4.hip, ivf_bin.hip) share, once: the work
// item of a workgroup, the gather of a group's query rows with its cut at the end of a row, and the scattered epilogue.
//
// A scan is strip_stream.h's pipeline cut LIST-MAJOR: a workgroup takes up to 256 consecutive rows of ONE list (a tile)
// against a group of up to 32 of the queries that probe that list (ivf.hip says why).  Workgroup b serves list l with
// item_off[l] <= b < item_off[l + 1]; its place there is tile * groups + group, groups = the 32-pair groups of the list.
// pair_off [nlist + 1] is the CSR of the (query, slot) pairs by list, pair_q / pair_col the query and the first output
// column of every pair.
//
// What a kernel adds: its stage geometry, the database side of an issue and where the query chunks go, its slab
// multiply, the numerator of a score.
#pragma once
#include "strip_stream.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kIvfQG = 32;                   // query rows per group = one 32 x 32 accumulator block
static constexpr int kIvfSub = kIvfQG * kStripRow;  // 4096: the 32 query rows of a group, 128 bytes each

// ---- the work item -----------------------------------------------------------------------------------------------------
// Every field is workgroup-uniform.  `valid` is false for a workgroup without work (one at or past item_off[nlist]: the
// grid may be any upper bound; a tile past the list's rows): the KERNEL returns on it, first thing, so every wave takes
// the same way out ahead of the first ring_barrier().
struct IvfItem {
    int l = 0, p0 = 0, p1 = 0;           // the list and its pairs
    int tile = 0, grp = 0, pbase = 0;    // the tile of 256 rows, the group of 32 pairs and its first pair
    int first = 0, iend = 0;             // the list's first row and its end (within NP)
    int i0 = 0, rows = 0;                // the tile's first row and how many rows it has
    bool valid = false;

    __device__ __forceinline__ IvfItem(int bid, const int* __restrict__ item_off, int nlist, const int* __restrict__ pair_off,
                                       const int* __restrict__ list_off, int NP) {
        // the last l with item_off[l] <= bid
        int lo = 0, hi = nlist;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (item_off[mid] <= bid) lo = mid; else hi = mid;
        }
        l = lo;
        p0 = pair_off[l], p1 = pair_off[l + 1];
        const int groups = (p1 - p0 + kIvfQG - 1) / kIvfQG;
        const int local = bid - item_off[l];
        if (groups <= 0 || local < 0) return;
        tile = local / groups, grp = local - tile * groups;
        first = list_off[l];
        i0 = first + tile * kStripRows;
        iend = min(list_off[l + 1], NP);
        rows = min(kStripRows, iend - i0);
        pbase = p0 + grp * kIvfQG;
        valid = i0 >= 0 && rows > 0;
    }
    // the row of a consumer lane: its place in the list, and in the database (stored only where n < iend)
    __device__ __forceinline__ int r(int wave, const StripLane& L) const { return tile * kStripRows + wave * 32 + L.lrow; }
    __device__ __forceinline__ int n(int r_) const { return first + r_; }
    // the query of group row `row`, or -1 for an empty row of the group and for a table entry outside [0, Q)
    __device__ __forceinline__ int query(const int* __restrict__ pair_q, int row, int Q) const {
        if (pbase + row >= p1) return -1;
        const int q = pair_q[pbase + row];
        return (unsigned)q < (unsigned)Q ? q : -1;
    }
};

// ---- the query side of a loader wave -----------------------------------------------------------------------------------
// Loader lw brings piece lw = rows 8 lw .. 8 lw + 7 of the group: row r is the query of pair pbase + r, gathered where it
// lies by a per-lane row offset (kOOB, so zeros, for an empty row).  The cut: a 16-byte chunk whose first byte in the
// query row is at or past Kq, the bytes of query codes in a row, is asked for at kOOB - the query pitch need not cover a
// slab and the scalar offset takes no part in the range check, so an uncut lane would read the next query's codes.
// Kq is a multiple of 32 and a chunk starts at a multiple of 16 below the end of the last slab, so this is the int8
// scan's "upper half of a last half slab", the fp4 scan's "chunk >= keep of the last slab" and the bit scan's "sub-image
// past what is left" for every admissible D; earlier slabs end at or below Kq and are never cut.
struct IvfQueryLane {
    uint32_t voff = kOOB;
    int left;                // Kq - the place of this lane's chunk in a stage row: a chunk `soff` on is cut when soff >= left
    int lw;

    __device__ __forceinline__ IvfQueryLane(const IvfItem& it, const int* __restrict__ pair_q, int Q, int ldq, int Kq, int lw_,
                                            int lane)
        : left(Kq - strip_piece_chunk(lw_, lane) * 16), lw(lw_) {
        const int q = it.query(pair_q, strip_piece_row(lw_, lane), Q);
        if (q >= 0) voff = (uint32_t)q * (uint32_t)ldq + (uint32_t)strip_piece_chunk(lw_, lane) * 16u;
    }
    // this wave's piece of the 32 x 128 bytes that start `soff` bytes into the query rows, to the sub-image at `sub`
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsrc, char* sub, int soff) const {
        dma16(rsrc, sub + lw * kStripPiece, soff >= left ? kOOB : voff, soff);
    }
};

// ---- the scattered epilogue --------------------------------------------------------------------------------------------
// Accumulator element j of a consumer lane is (group row L.qrow(0, j >> 2) + (j & 3), the lane's database row): its score
// goes to column pair_col + r of the pair's query, in three rounds of independent loads (query and column; scale and,
// with SUMS, the query's code sum; then the stores).  num(j, su) is the numerator of element j as a float.
template <bool SUMS, class Num>
__device__ __forceinline__ void ivf_scatter(const IvfItem& it, const StripLane& L, int r, const int* __restrict__ pair_q,
                                            const int* __restrict__ pair_col, const float* __restrict__ qscales,
                                            const int* __restrict__ qsums, int Q, const float* __restrict__ bscales,
                                            const int* __restrict__ ids, float* __restrict__ out, int* __restrict__ out_ids,
                                            int ldo, int width, Num&& num) {
    const int n = it.n(r);
    if (n >= it.iend) return;
    const float sb = bscales[n];
    const int id = ids[n];
    int qv[16];
    long cv[16];
    float sq[16];
    int su[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int pi = it.pbase + L.qrow(0, j >> 2) + (j & 3);
        const bool ok = pi < it.p1;
        qv[j] = ok ? pair_q[pi] : -1;
        cv[j] = ok ? (long)pair_col[pi] + r : -1;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if ((unsigned)qv[j] >= (unsigned)Q || cv[j] >= width) cv[j] = -1;        // a table that does not fit: no store
        sq[j] = cv[j] >= 0 ? qscales[qv[j]] : 0.f;
        su[j] = SUMS && cv[j] >= 0 ? qsums[qv[j]] : 0;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (cv[j] >= 0) {
            out[(size_t)qv[j] * ldo + cv[j]] = __fmul_rn(__fmul_rn(num(j, su[j]), sq[j]), sb);
            out_ids[(size_t)qv[j] * ldo + cv[j]] = id;
        }
}

}  // namespace dir

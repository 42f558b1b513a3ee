// ivf_fp4.hip — the inverted file over fp4 codes: the scan of the probed lists on the scaled matrix cores.
//
// ivf.hip reads only the lists a query falls into, at 2048 + 4 bytes a row of 2048; index_fp4.hip halves the row and reads
// all of them.  ivf_scan_fp4_kernel is ivf_scan_i8_kernel's cut - list-major, a workgroup takes up to 256 consecutive rows
// of ONE list against a group of up to 32 of the queries that probe it, the same probe tables, the same work items, four
// stages - with sim_fp4_kernel's arithmetic: a stage row of 128 bytes is 256 k of e2m1 codes, a slab is four
// v_mfma_scale_f32_32x32x64_f8f6f4 steps into one f32x16 accumulator block, and acc is exact (include/dir_engine.h), so a
// score is dir_similarity_fp4's number whatever the cut.
//   Database side: ChunkCutLoader as the flat scan runs it (the last slab cut by 16-byte chunk), the descriptor based at the
//     tile's first row; the row's 8 block bytes of a slab come from one 8-byte global load per consumer lane, one slab ahead.
//   Query side: the 32 rows of a group are gathered where they lie by a per-lane row offset from the pair table (kOOB
//     for an empty row of the group), cut by chunk in the last slab as well: the query pitch is pad64(D) / 2 and need not
//     cover a slab, so an uncut lane would read the next query's codes.  There is no image for the block bytes to ride in
//     (a group is a gather, not a block of consecutive queries), and through the stage they would be 256 bytes a slab in
//     8-byte pieces: a DMA instruction for 1/144 of the bytes.  They take the database side's path instead: consumer lane
//     (lrow, lhi) loads the 8 bytes of the slab of query pair_q[pbase + lrow] from global memory, one slab ahead, and
//     picks bytes 2 s + lhi.  Both loads of a slab hide behind the slab's MFMAs.
//   Bytes of blocks past pad64(D) are forced to 127 on both sides, as are all of an empty group row: the codes there are
//     the zeros an out-of-range DMA lane writes, and 0 x 2^0 adds nothing, where a stray 0xFF byte would make a NaN.
// LDS: 4 stages x (32 768 database + 4096 query codes) = 147 456 of 163 840 bytes.  92 VGPRs (three waves a SIMD allow 168), no
// atomics, no scratch.
#include "dir_common.h"
#include "ivf_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the score is defined in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kIvfFp4Stage = kStripSlab + kIvfSub;   // 36864
static constexpr int kIvfFp4Stages = 4;                // three slabs in flight, one being multiplied
static constexpr int kIvfFp4Lds = kIvfFp4Stages * kIvfFp4Stage;           // 147456 of 163840

// The work item, the query gather and the epilogue: ivf_scan.h.
__global__ void __launch_bounds__(768) ivf_scan_fp4_kernel(const uint8_t* __restrict__ qcodes, int ldq, const uint8_t* __restrict__ QE,
                                                          int ldqe, const float* __restrict__ qscales, int Q,
                                                          const uint8_t* __restrict__ P, int ldp, const uint8_t* __restrict__ PE,
                                                          int ldpe, const float* __restrict__ bscales, const int* __restrict__ ids,
                                                          int NP, int Kb, int T, const int* __restrict__ list_off, int nlist,
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
        const __amdgpu_buffer_rsrc_t rsrc_p = buffer_rsrc(P + (size_t)it.i0 * ldp, (uint32_t)(((size_t)it.rows - 1) * ldp + Kb));
        const __amdgpu_buffer_rsrc_t rsrc_q = buffer_rsrc(qcodes, (uint32_t)(((size_t)Q - 1) * ldq + Kb));
        const ChunkCutLoader db(lw, lane, (uint32_t)ldp, Kb, T);
        const IvfQueryLane qs(it, pair_q, Q, ldq, Kb, lw, lane);
        strip_load<kIvfFp4Stage, kIvfFp4Stages, 9>(smem, T, rot, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
            qs.issue(rsrc_q, stage + kStripSlab, u * kStripRow);
        });
        return;
    }

    const StripLane L(wave, lane);
    const int r = it.r(wave, L), n = it.n(r);
    // the block bytes: 8 per slab and row, one slab ahead, on both sides (a row past the list reads the list's last row's:
    // its scores are not stored; an empty row of the group multiplies zeros under 127)
    const uint8_t* erow = PE + (size_t)min(n, it.iend - 1) * ldpe;
    const int qmine = it.query(pair_q, L.lrow, Q);
    const uint8_t* qerow = QE + (size_t)max(qmine, 0) * ldqe;
    const uint32_t qnone = qmine < 0 ? 0xffffffffu : 0u;
    // byte s of a step's scale dword is block 2 s + lhi of the slab; in the last slab the blocks past Kb hold 127
    const int lastb = (Kb >> 4) - (T - 1) * 8;
    uint32_t pad = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) pad |= (s * 2 + L.lhi >= lastb ? 0xffu : 0u) << (8 * s);
    f32x16_t acc[1] = {};
    const int u0 = strip_slab(0, rot, T);
    u32x2_t nxt_b = *(const u32x2_t*)(erow + 8 * u0);
    u32x2_t nxt_q = *(const u32x2_t*)(qerow + 8 * u0);
    int t = 0;
    strip_consume<kIvfFp4Stage, kIvfFp4Stages>(smem, T, rot, [&](const char* stage, int u) __attribute__((always_inline)) {
        const u32x2_t cur_b = nxt_b, cur_q = nxt_q;
        if (++t < T) {
            const int un = strip_slab(t, rot, T);
            nxt_b = *(const u32x2_t*)(erow + 8 * un);
            nxt_q = *(const u32x2_t*)(qerow + 8 * un);
        }
        uint32_t eb = fp4_pick_bytes(cur_b, L.lhi);
        uint32_t eq = fp4_pick_bytes(cur_q, L.lhi);
        const uint32_t cut = u == T - 1 ? pad : 0u;
        eb = (eb & ~cut) | (0x7f7f7f7fu & cut);
        const uint32_t qcut = cut | qnone;
        eq = (eq & ~qcut) | (0x7f7f7f7fu & qcut);
        const uint32_t aexp[1] = {eq};
        fp4_slab_mma<1>(L, stage, aexp, eb, acc);
    });
    ivf_scatter<false>(it, L, r, pair_q, pair_col, qscales, nullptr, Q, bscales, ids, out, out_ids, ldo, width,
                       [&](int j, int) __attribute__((always_inline)) { return acc[0][j]; });
}

// the scan's admission rules beyond the sizes (c_api.hip reports them): ivf_scan_admissible for the codes; one aligned
// 8-byte load of block bytes per slab and row on both sides, so their pitches cover whole slabs
bool ivf_scan_fp4_admissible(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, int Q, const uint8_t* bcodes,
                             int ldb, const uint8_t* bexps, int ldbe, int D) {
    return ivf_scan_admissible(qcodes, ldq, Q, bcodes, ldb) && ((ldqe | ldbe) & 7) == 0 &&
           ((((uintptr_t)qexps) | ((uintptr_t)bexps)) & 7) == 0 && ldqe >= fp4_exp_bytes(D) && ldbe >= fp4_exp_bytes(D);
}

int ivf_scan_fp4(const uint8_t* qcodes, int ldq, const uint8_t* qexps, int ldqe, const float* qscales, int Q,
                 const uint8_t* bcodes, int ldb, const uint8_t* bexps, int ldbe, const float* bscales, const int* ids, int N,
                 int D, const int* list_off, int nlist, const int* pair_off, const int* pair_q, const int* pair_col,
                 const int* item_off, int items, float* scores, int* out_ids, int lds, int width, hipStream_t stream) {
    if (Q <= 0 || width <= 0) return DIR_OK;
    DIR_CHECK(ivf_scan_begin("ivf_scan_fp4", Q, width, items, out_ids, lds, stream));
    if (items <= 0 || N <= 0) return DIR_OK;
    const int Kb = pad64(D) / 2, T = fp4_slabs(D);
    static std::atomic<uint64_t> attr_done{0};
    DIR_HIP_CHECK(ensure_dynamic_lds((const void*)ivf_scan_fp4_kernel, kIvfFp4Lds, attr_done));
    hipLaunchKernelGGL(ivf_scan_fp4_kernel, dim3((unsigned)items), dim3(768), kIvfFp4Lds, stream, qcodes, ldq, qexps, ldqe, qscales,
                       Q, bcodes, ldb, bexps, ldbe, bscales, ids, N, Kb, T, list_off, nlist, pair_off, pair_q, pair_col,
                       item_off, scores, out_ids, lds, width);
    DIR_HIP_CHECK(hipGetLastError());
    return DIR_OK;
}

}  // namespace dir

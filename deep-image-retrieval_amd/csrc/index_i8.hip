// index_i8.hip — the int8 descriptor index: quantise rows, scan the codes on the int8 matrix cores, re-score a shortlist.
//
// The fp32 database is the whole cost of a similarity pass at 10^6 rows (sim_split.hip: 8.2 GB per query block at
// 1 006 322 x 2048).  A per-row int8 code with one fp32 scale per row (include/dir_engine.h gives the definition) is a
// quarter of the bytes, and an int8 dot product accumulated in int32 is EXACT: a quantised score
//     scores[q][n] = ((float)dot_i32 * qscales[q]) * bscales[n]
// is one defined fp32 number whatever the tiling, the K order, the chunking or the sharding, so the ranked lists that
// come out of a scan cannot depend on how the caller cut the work.  Search then takes the usual two steps: the scan keeps
// a shortlist per query (topk.hip), gather_scores re-scores the shortlist against the fp32 rows.
//
// sim_i8_kernel runs strip_stream.h's pipeline with codes in the stages: one 768-thread workgroup per 256 database rows;
// the consumer waves multiply a 32-row strip each against a block of 96 query rows (three int32 accumulator blocks of
// v_mfma_i32_32x32x32_i8).  A 128-byte stage row holds 128 k, so a K slab is 128 wide: 32 KB of database codes + the
// 12 KB query image of the slab, prepared once by code_image_kernel as an image of the LDS stage and re-streamed from
// L2.  Three stages, two in flight; further query blocks on grid.y.  Rows are padded to 64 and not to a slab, hence the
// loader's half-slab cut.  Bytes per launch: N * ldb (codes, once per query block) + Q * N * 4 (scores).
#include "dir_common.h"
#include "flat_scan.h"
#include "pointwise.h"

#pragma clang fp contract(off)   // the definition is in single IEEE operations: nothing here may fuse

namespace dir {

static constexpr int kI8MaxDim = 131072;          // 127 * 127 * 131072 = 2 114 060 288 < 2^31
static constexpr int kI8SlabQ = kQB * kStripRow;      // 12288
static constexpr int kI8Stage = kStripSlab + kI8SlabQ;
static constexpr int kI8Stages = 3;
static constexpr int kI8Lds = kI8Stages * kI8Stage;   // 135168 of 163840

int index_i8_max_dim() { return kI8MaxDim; }

// ---- quantisation ------------------------------------------------------------------------------------------------------
// One wave per row, a lane owns quads of consecutive k: quad (c * 8 + i) * 64 + lane of chunk c (2048 values).  A row of
// up to 2048 values stays in registers between the amax pass and the rounding pass; a wider row is read twice.
__global__ void __launch_bounds__(256) quantize_rows_i8_kernel(const float* __restrict__ X, int ldx, int N, int D,
                                                             int8_t* __restrict__ codes, int ldc,
                                                             float* __restrict__ scales) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* row = X + (size_t)n * ldx;
    const bool vec = (ldx & 3) == 0 && (((uintptr_t)X) & 15) == 0;
    const int Dp = pad64(D);
    const int chunks = (D + 2047) >> 11;
    f32x4_t v[8];
    float amax = 0.f;
    bool bad = false;
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[i] = load4_guarded(row, ((c * 8 + i) * 64 + lane) * 4, D, vec);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float xe = v[i][e];     // (a copy: __builtin_bit_cast of a vector ELEMENT reads element 0)
                const uint32_t b = __builtin_bit_cast(uint32_t, xe) & 0x7fffffffu;
                bad |= b >= 0x7f800000u;                              // an infinity or a NaN
                amax = fmaxf(amax, __builtin_bit_cast(float, b));     // (fmaxf drops a NaN: `bad` keeps it)
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d));
    bad = __any(bad);
    float scale = __fdiv_rn(amax, 127.f);
    float inv = __fdiv_rn(127.f, amax);
    const bool zero = bad || !(inv <= 3.4028234663852886e38f);        // amax zero or tiny: 127 / amax overflows
    if (zero) inv = 0.f, scale = bad ? __builtin_nanf("") : 0.f;
    int8_t* crow = codes + (size_t)n * ldc;
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = ((c * 8 + i) * 64 + lane) * 4;
            if (k >= Dp) continue;
            if (chunks > 1) v[i] = load4_guarded(row, k, D, vec);
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float r = rintf(__fmul_rn(v[i][e], inv));             // round half to even
                r = fminf(fmaxf(r, -127.f), 127.f);
                const int code = (zero || k + e >= D) ? 0 : (int)r;
                w |= ((uint32_t)code & 0xffu) << (8 * e);
            }
            *(uint32_t*)(crow + k) = w;                               // (k % 4 == 0, ldc % 4 == 0, codes 4-byte aligned)
        }
    }
    if (lane == 0) scales[n] = scale;
}

int quantize_rows_i8(const float* X, int ldx, int N, int D, int8_t* codes, int ldc, float* scales, hipStream_t stream) {
    return rows_launch("quantize_rows_i8", "N", N, [&](unsigned blocks) {
        hipLaunchKernelGGL(quantize_rows_i8_kernel, dim3(blocks), dim3(256), 0, stream, X, ldx, N, D, codes, ldc, scales);
    });
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
// Query codes as an image of the LDS stages: [query block][K slab of 128][96 rows][128 bytes], the eight 16-byte chunks
// of a row XOR-swizzled by (row >> 1) & 7 - the swizzle of the database rows.  Rows past Q and k past D are zero, so
// whatever the database holds beyond D multiplies a zero.
__global__ void __launch_bounds__(256) code_image_kernel(const int8_t* __restrict__ qcodes, int ldq, int Q, int D,
                                                       int8_t* __restrict__ img) {
    const int t = blockIdx.x, qb = blockIdx.y, T = gridDim.x;
    int8_t* dst = img + ((size_t)qb * T + t) * kI8SlabQ;
    for (int item = threadIdx.x; item < kQB * 8; item += 256) {
        const int row = item >> 3, pos = item & 7;
        const int chunk = strip_chunk(pos, row);
        const int q = qb * kQB + row;
        const int k0 = t * kStripRow + chunk * 16;
        u32x4_t w = {0u, 0u, 0u, 0u};
        if (q < Q) {
            const int8_t* src = qcodes + (size_t)q * ldq + k0;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                if (k0 + e < D) w[e >> 2] |= ((uint32_t)(uint8_t)src[e]) << (8 * (e & 3));
        }
        *(u32x4_t*)(dst + row * 128 + pos * 16) = w;
    }
}

// the image of Q rows as qblocks blocks of T slabs (index_bin.hip streams the same image)
hipError_t code_image(const int8_t* qcodes, int ldq, int Q, int D, int8_t* img, int T, int qblocks, hipStream_t stream) {
    hipLaunchKernelGGL(code_image_kernel, dim3(T, qblocks), dim3(256), 0, stream, qcodes, ldq, Q, D, img);
    return hipGetLastError();
}

__global__ void __launch_bounds__(768) sim_i8_kernel(const int8_t* __restrict__ P, int ldp, int NP, int Kp,
                                                    const int8_t* __restrict__ img, const float* __restrict__ qscales,
                                                    const float* __restrict__ bscales, float* __restrict__ out, int ldo,
                                                    int NQ, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const FlatFrame f(NP);
    const int rot = strip_rot(f.tile, T);

    if (wave >= 8) {
        const int lw = wave - 8;
        // Kp = D rounded up to 64 bytes of every row are readable
        const __amdgpu_buffer_rsrc_t rsrc_p = f.database(P, ldp, Kp), rsrc_q = f.image(img, T, kI8SlabQ);
        const StripLoader<true> db(lw, lane, (uint32_t)ldp, Kp, T);
        strip_load<kI8Stage, kI8Stages, 11>(smem, T, rot, [&](char* stage, int u) __attribute__((always_inline)) {
            db.issue(rsrc_p, stage, u);
#pragma unroll
            for (int i = 0; i < 3; ++i) strip_image_piece(rsrc_q, stage, lw * 3 + i, lane, u * kI8SlabQ);
        });
        return;
    }

    const StripLane L(wave, lane);
    i32x16_t acc[3] = {};
    strip_consume<kI8Stage, kI8Stages>(smem, T, rot, [&](const char* stage, int) __attribute__((always_inline)) {
        code_slab_mma<3>(L, stage, acc);
    });

    flat_store(f, L, f.n(wave, L), qscales, bscales, out, ldo, NQ,
               [&](int j, int i, int) __attribute__((always_inline)) { return (float)acc[j][i]; });
}

int similarity_i8(const int8_t* qcodes, int ldq, const float* qscales, int Q, const int8_t* bcodes, int ldb,
                  const float* bscales, int N, int D, float* scores, int lds, hipStream_t stream) {
    const int Kp = pad64(D), T = ceil_div(Kp, kStripRow), qblocks = ceil_div(Q, kQB);
    static std::atomic<uint64_t> attr_done{0};
    return flat_scan_launch(
        "similarity_i8", Q, N, (size_t)qblocks * T * kI8SlabQ, (const void*)sim_i8_kernel, kI8Lds, attr_done, stream,
        [&](char* img) { return code_image(qcodes, ldq, Q, D, (int8_t*)img, T, qblocks, stream); },
        [&](char* img, dim3 grid) {
            hipLaunchKernelGGL(sim_i8_kernel, grid, dim3(768), kI8Lds, stream, bcodes, ldb, N, Kp, (const int8_t*)img, qscales,
                               bscales, scores, lds, Q, T);
        });
}

// the flat scans' admission rules beyond the sizes (c_api.hip reports them): 16-byte pieces, one 2 GB descriptor per tile
bool flat_scan_admissible(const void* rows, int ldb) {
    return (ldb & 15) == 0 && (((uintptr_t)rows) & 15) == 0 && (size_t)ldb * kStripRows < (1ull << 31);
}

// ... and one 2 GB descriptor for the image of a query block
bool similarity_i8_admissible(const int8_t* bcodes, int ldb, int D) {
    return flat_scan_admissible(bcodes, ldb) && (size_t)ceil_div(pad64(D), kStripRow) * kI8SlabQ < (1ull << 31);
}

// ---- re-scoring a shortlist --------------------------------------------------------------------------------------------
// One wave per (query, candidate): fp32 products and sums (fmaf chain per lane over k = 256 i + 4 lane + e, then a
// butterfly), D / 64 + 6 roundings on the longest path.
__global__ void __launch_bounds__(256) gather_scores_kernel(const float* __restrict__ Qm, int ldq, const float* __restrict__ B,
                                                          int ldb, int D, const int* __restrict__ cand, int ldcand, int R,
                                                          float* __restrict__ scores, int ldsc, long item0, long total) {
    const int lane = threadIdx.x & 63;
    const long item = item0 + (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= total) return;
    const int q = (int)(item / R), r = (int)(item % R);
    const int c = cand[(size_t)q * ldcand + r];
    float acc = 0.f;
    if (c >= 0) {
        const float* x = Qm + (size_t)q * ldq;
        const float* y = B + (size_t)c * ldb;
        const bool vec = ((ldq | ldb) & 3) == 0 && ((((uintptr_t)Qm) | ((uintptr_t)B)) & 15) == 0;
        for (int k = lane * 4; k < D; k += 256) {
            if (vec && k + 3 < D) {
                const f32x4_t a = *(const f32x4_t*)(x + k), b = *(const f32x4_t*)(y + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc = __builtin_fmaf(a[e], b[e], acc);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < D) acc = __builtin_fmaf(x[k + e], y[k + e], acc);
            }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    } else {
        acc = __builtin_nanf("");
    }
    if (lane == 0) scores[(size_t)q * ldsc + r] = acc;
}

int gather_scores(const float* queries, int ldq, int Q, const float* database, int ldb, int D, const int* cand, int ldcand,
                  int R, float* scores, int ldsc, hipStream_t stream) {
    if (Q <= 0 || R <= 0) return DIR_OK;
    // the pairs are independent: as many launches of at most kMaxLaunchThreads threads as Q * R asks for, launch i from
    // pair i * kGatherMaxBlocks * 4 (a pair's wave and its order of operations do not depend on the cut)
    constexpr long kGatherMaxBlocks = kMaxLaunchThreads / 256;
    const long total = (long)Q * R, blocks = (total + 3) / 4;
    for (long b0 = 0; b0 < blocks; b0 += kGatherMaxBlocks) {
        const long nb = blocks - b0 < kGatherMaxBlocks ? blocks - b0 : kGatherMaxBlocks;
        hipLaunchKernelGGL(gather_scores_kernel, dim3((unsigned)nb), dim3(256), 0, stream, queries, ldq, database, ldb, D, cand,
                           ldcand, R, scores, ldsc, b0 * 4, total);
        DIR_HIP_CHECK(hipGetLastError());
    }
    return DIR_OK;
}

}  // namespace dir

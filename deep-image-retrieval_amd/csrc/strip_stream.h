// strip_stream.h — the row-strip LDS-DMA pipeline of the scan kernels (sim_split.hip, index_i8.hip, index_fp4.hip,
// index_bin.hip, and through ivf_scan.h the list-major scans ivf.hip, ivf_fp4.hip, ivf_bin.hip), once.
//
// One workgroup per 256 database rows.  Eight consumer waves own a 32-row strip each and multiply it against the query
// rows of the stage; four loader waves (8 .. 11) only issue LDS-DMA and wait for it.  A stage is 32 KB of database (256
// rows of 128 bytes = one K slab, raw from HBM, each byte used by exactly one wave) followed by the kernel's query
// part; the eight 16-byte chunks of a stage row are XOR-swizzled by (row >> 1) & 7, so a wave's fragment reads spread
// over all banks.  STAGES stages form a ring with STAGES - 1 slabs in flight, and one ring_barrier() per slab is the
// hand-off both ways: slab t has landed everywhere / everyone has left slab t - 1, whose slot is free.  Every workgroup
// walks K from its own starting slab (strip_rot): with a multi-KiB row pitch workgroups in lock-step would all be on
// the same few HBM channels at any instant.
//
// What a kernel adds: its block decode, its buffer descriptors, the query side of an issue, its epilogue.
#pragma once
#include "dir_common.h"
#include "conv_device.h"

namespace dir {

static constexpr int kStripRows = 256;                 // database rows per workgroup
static constexpr int kStripRow = 128;                  // bytes of a stage row = bytes of a K slab in a database row
static constexpr int kStripSlab = kStripRows * kStripRow;   // 32768: the database part of a stage; the query part follows
static constexpr int kStripPiece = 1024;               // one LDS-DMA instruction: 64 lanes x 16 bytes = 8 stage rows
static constexpr float kPairScale = 1024.f;            // 2^10: |x| < 64 stays finite in fp16, unit-vector entries mid-range

// ---- stage geometry ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ int strip_rot(int tile, int T) { return (int)(((unsigned)tile * 7u) % (unsigned)T); }
// the K slab of step t (the sum is the same in any order: exact products, and the tests pin the fp32 bits)
__device__ __forceinline__ int strip_slab(int t, int rot, int T) {
    const int u = t + rot;
    return u >= T ? u - T : u;
}
// where chunk c of stage row `row` lies in the row
__device__ __forceinline__ int strip_chunk(int c, int row) { return c ^ ((row >> 1) & 7); }
// piece j holds stage rows 8j .. 8j+7, 8 lanes x 16 bytes per row: the row and the source chunk of this lane
__device__ __forceinline__ int strip_piece_row(int j, int lane) { return j * 8 + (lane >> 3); }
__device__ __forceinline__ int strip_piece_chunk(int j, int lane) { return strip_chunk(lane & 7, strip_piece_row(j, lane)); }
// ... and its buffer offset in a matrix of `pitch` bytes per row (rows past the descriptor: out of range -> zeros)
__device__ __forceinline__ uint32_t strip_piece_voff(int j, int lane, uint32_t pitch) {
    return (uint32_t)strip_piece_row(j, lane) * pitch + (uint32_t)strip_piece_chunk(j, lane) * 16u;
}

// piece p of a query image that is byte for byte the query part of a stage (a linear copy); soff: where slab u starts
__device__ __forceinline__ void strip_image_piece(__amdgpu_buffer_rsrc_t rsrc, char* stage, int p, int lane, int soff) {
    dma16(rsrc, stage + kStripSlab + p * kStripPiece, (uint32_t)(p * kStripPiece + lane * 16), soff);
}

template <int N, bool LGKM = false>
__device__ __forceinline__ void wait_vmcnt() {
    if constexpr (LGKM)
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"i"(N) : "memory");
    else
        asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// ---- the database side of a loader wave --------------------------------------------------------------------------------
// Loader lw (0 .. 3) brings pieces 8 lw .. 8 lw + 7 of every slab.  HALF_CUT (the int8 scans, whose rows are padded to 64
// and not to a slab): when Kp % 128 == 64 the upper half of the last slab lies past Kp, and as the scalar offset takes no
// part in the range check those lanes ask for an address that is out of range by itself.
template <bool HALF_CUT>
struct StripLoader {
    uint32_t pvoff[8];
    uint32_t upper = 0;      // bit i: this lane's chunk of piece i lies in the upper 64 bytes of a slab
    int lw, last;            // last: the final slab where it is a half slab, or -1

    __device__ __forceinline__ StripLoader(int lw_, int lane, uint32_t pitch, int Kp = 0, int T = 0)
        : lw(lw_), last(HALF_CUT && (Kp & 64) ? T - 1 : -1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            pvoff[i] = strip_piece_voff(lw * 8 + i, lane, pitch);
            upper |= (uint32_t)(strip_piece_chunk(lw * 8 + i, lane) >= 4) << i;
        }
    }
    __device__ __forceinline__ bool cut(int u) const { return HALF_CUT && u == last; }
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsrc, char* stage, int u) const {
        const bool c = cut(u);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            dma16(rsrc, stage + (lw * 8 + i) * kStripPiece, (c && ((upper >> i) & 1u)) ? kOOB : pvoff[i], u * kStripRow);
    }
};

// ---- the loader loop ---------------------------------------------------------------------------------------------------
// issue(stage, u) puts slab u into `stage` with OPS LDS-DMA instructions of this wave (OPS_ALT where `alt`: a kernel whose
// loaders carry unequal shares).  Before hand-off t this wave's part of slab t has landed; the OPS ops of each of the up
// to STAGES - 2 newer slabs may stay in flight.  LGKM: the wait also covers the wave's own LDS writes.
template <int AHEAD, int OPS, int OPS_ALT, bool LGKM>
__device__ __forceinline__ void strip_wait(int t, int T, bool alt) {
    if constexpr (AHEAD == 0) {
        wait_vmcnt<0, LGKM>();
    } else if (t + AHEAD < T) {
        if (OPS_ALT != OPS && alt)
            wait_vmcnt<AHEAD * OPS_ALT, LGKM>();
        else
            wait_vmcnt<AHEAD * OPS, LGKM>();
    } else {
        strip_wait<AHEAD - 1, OPS, OPS_ALT, LGKM>(t, T, alt);
    }
}

template <int STAGE, int STAGES, int OPS, int OPS_ALT = OPS, bool LGKM = false, class Issue>
__device__ __forceinline__ void strip_load(char* smem, int T, int rot, Issue&& issue, bool alt = false) {
    auto put = [&](int t) __attribute__((always_inline)) { issue(smem + (t % STAGES) * STAGE, strip_slab(t, rot, T)); };
#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
        if (p == 0 || T > p) put(p);
    for (int t = 0; t < T; ++t) {
        strip_wait<STAGES - 2, OPS, OPS_ALT, LGKM>(t, T, alt);
        ring_barrier();   // hand-off t: slab t is complete; the consumers have left slab t - 1
        if (t + STAGES - 1 < T) put(t + STAGES - 1);
    }
}

// ---- the consumer loop -------------------------------------------------------------------------------------------------
template <int STAGE, int STAGES, class Body>
__device__ __forceinline__ void strip_consume(const char* smem, int T, int rot, Body&& body) {
    int cur = 0;
    for (int t = 0; t < T; ++t) {
        ring_barrier();   // hand-off t (see strip_load)
        body(smem + cur * STAGE, strip_slab(t, rot, T));
        cur = cur + 1 == STAGES ? 0 : cur + 1;
    }
}

// A consumer lane's place: database row lrow of its wave's strip; lhi picks the k half of an MFMA step.
struct StripLane {
    int lrow, lhi, boff;
    __device__ __forceinline__ StripLane(int wave, int lane) : lrow(lane & 31), lhi(lane >> 5), boff((wave * 32 + lrow) * kStripRow) {}
    // byte offset of chunk c in the lane's row (a query row 32 j + lrow has the same swizzle) / of that chunk of the database row
    __device__ __forceinline__ int chunk(int c) const { return strip_chunk(c, lrow) << 4; }
    __device__ __forceinline__ int b(int c) const { return boff + chunk(c); }
    // the epilogue: accumulator element 4 g + e of block j is (query row qrow(j, g) + e, database row lrow)
    __device__ __forceinline__ int qrow(int j, int g) const { return 32 * j + 8 * g + 4 * lhi; }
};

// ---- fp32 operands as 16-bit planes ------------------------------------------------------------------------------------
// x0, x1 -> packed bf16 planes (low half = x0): x = h + m + l
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& h, uint32_t& m, uint32_t& l) {
    float a, b;
    h = BF16::pack(x0, x1);
    BF16::unpack(h, a, b);
    x0 -= a, x1 -= b;
    m = BF16::pack(x0, x1);
    BF16::unpack(m, a, b);
    x0 -= a, x1 -= b;
    l = BF16::pack(x0, x1);
}
// x0, x1 (already scaled by 2^10) -> packed fp16 planes: x = h + l
__device__ __forceinline__ void split2h(float x0, float x1, uint32_t& h, uint32_t& l) {
    float a, b;
    h = FP16::pack(x0, x1);
    FP16::unpack(h, a, b);
    l = FP16::pack(x0 - a, x1 - b);
}

static constexpr int kQB = 96;                         // query rows per block: three 32 x 32 accumulator blocks
static constexpr int kPlane = kQB * 64;                // bytes of one 16-bit plane of a 32-wide K slab
__host__ __device__ constexpr int plane_slab(bool pair) { return (pair ? 2 : 3) * kPlane; }   // query part of a stage
__host__ __device__ constexpr int plane_stage(bool pair) { return kStripSlab + plane_slab(pair); }

// The plain transform of the raw database values before the split: the 2^10 scale of the PAIR form, nothing otherwise.
template <bool PAIR>
struct PairScale {
    __device__ __forceinline__ void operator()(f32x4_t& b0, f32x4_t& b1, int, int) const {
        if constexpr (PAIR) {
#pragma unroll
            for (int e = 0; e < 4; ++e) b0[e] *= kPairScale, b1[e] *= kPairScale;
        }
    }
};

// One 32-wide fp32 K slab of a stage whose query part is the plane image [plane][96 rows][64 bytes] (four chunks per row
// swizzled by (row >> 2) & 3): the lane's 16 database values are read, transformed by pre(b0, b1, u, c0) (their k is
// 32 u + 4 c0 + 0..7), split into planes and multiplied.  !PAIR: three bf16 planes, six products; PAIR: two fp16 planes
// of 2^10 x, three products.  The corrections (weight <= 2^-8) go to `lo`, the leading product to `acc`: the leading sum
// sees K/16 roundings, and the two meet once in the epilogue.  The order of products and accumulators is part of the result.
template <bool PAIR, class Pre>
__device__ __forceinline__ void plane_slab_mma(const StripLane& L, const char* stage, int u, Pre&& pre, f32x16_t (&acc)[3],
                                               f32x16_t (&lo)[3]) {
    const int aoff = kStripSlab + L.lrow * 64, aswz = (L.lrow >> 2) & 3;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int c0 = s * 4 + L.lhi * 2;
        f32x4_t b0 = *(const f32x4_t*)(stage + L.b(c0));
        f32x4_t b1 = *(const f32x4_t*)(stage + L.b(c0 + 1));
        pre(b0, b1, u, c0);
        u32x4_t ah[3], am[3], al[3];
        const int ach = ((s * 2 + L.lhi) ^ aswz) << 4;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            ah[j] = *(const u32x4_t*)(stage + aoff + 0 * kPlane + j * 2048 + ach);
            am[j] = *(const u32x4_t*)(stage + aoff + 1 * kPlane + j * 2048 + ach);
            if (!PAIR) al[j] = *(const u32x4_t*)(stage + aoff + 2 * kPlane + j * 2048 + ach);
        }
        u32x4_t bh, bm, bl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            uint32_t h, m, l = 0;
            const float x0 = e < 2 ? b0[2 * e] : b1[2 * e - 4], x1 = e < 2 ? b0[2 * e + 1] : b1[2 * e - 3];
            if (PAIR)
                split2h(x0, x1, h, m);
            else
                split2(x0, x1, h, m, l);
            bh[e] = h, bm[e] = m, bl[e] = l;
        }
        if constexpr (PAIR) {   // planes (h, m) = (hi, lo) of fp16
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                lo[j] = FP16::mfma32(__builtin_bit_cast(f16x8_t, am[j]), __builtin_bit_cast(f16x8_t, bh), lo[j]);
                lo[j] = FP16::mfma32(__builtin_bit_cast(f16x8_t, ah[j]), __builtin_bit_cast(f16x8_t, bm), lo[j]);
                acc[j] = FP16::mfma32(__builtin_bit_cast(f16x8_t, ah[j]), __builtin_bit_cast(f16x8_t, bh), acc[j]);
            }
        } else {
            auto mm = [&](f32x16_t (&c)[3], const u32x4_t (&a)[3], const u32x4_t& b) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = BF16::mfma32(__builtin_bit_cast(bf16x8_t, a[j]), __builtin_bit_cast(bf16x8_t, b), c[j]);
            };
            mm(lo, al, bh);
            mm(lo, ah, bl);
            mm(lo, am, bm);
            mm(lo, am, bh);
            mm(lo, ah, bm);
            mm(acc, ah, bh);
        }
    }
}

// ---- int8 codes --------------------------------------------------------------------------------------------------------
// One 128-wide K slab of a stage whose query part is NB blocks of 32 rows x 128 bytes, swizzled like the database rows
// (query row 32 j + lrow has lrow's swizzle).  Both operands of a step are the same 16 consecutive bytes of a row per
// lane, so whatever k order the instruction gives the 16 bytes of a lane half is the same on both sides.
template <int NB>
__device__ __forceinline__ void code_slab_mma(const StripLane& L, const char* stage, i32x16_t (&acc)[NB]) {
    const int aoff = kStripSlab + L.lrow * kStripRow;
#pragma unroll
    for (int s = 0; s < 4; ++s) {         // k = 128 u + 32 s + 16 lhi + 0..15
        const int ch = L.chunk(s * 2 + L.lhi);
        const i32x4_t b = *(const i32x4_t*)(stage + L.boff + ch);
#pragma unroll
        for (int j = 0; j < NB; ++j)
            acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4_t*)(stage + aoff + j * 4096 + ch), b, acc[j], 0, 0, 0);
    }
}

// ---- fp4 codes ---------------------------------------------------------------------------------------------------------
// One 256-wide K slab of a stage of e2m1 codes (two k per byte): the query part is NB blocks of 32 rows x 128 bytes,
// swizzled like the database rows, then [2 lane halves][NB * 32 rows] dwords of e8m0 block bytes.  A lane's operand of
// step s is chunk 2 s + lhi of its row = one block of 32 k on both sides, so the k order inside the lane does not matter;
// its scales are byte s of `bexp` (the database row's, from the caller) and of the query row's dword for this lane half.
typedef __attribute__((ext_vector_type(8))) int i32x8_t;

static constexpr int kFp4SlabK = 2 * kStripRow;    // 256 k in a stage row
__host__ __device__ inline int fp4_slabs(int D) { return (pad64(D) + kFp4SlabK - 1) / kFp4SlabK; }
// bytes of block bytes in a row: 8 per slab, whole slabs (the codes of a row are pad64(D) / 2 bytes)
__host__ __device__ inline int fp4_exp_bytes(int D) { return 8 * fp4_slabs(D); }

// The database side of a loader wave: StripLoader's pieces with a cut by chunk.  Kb (bytes of codes in a row, a multiple
// of 32; of 16 for rows of bits) leaves 2, 4, 6 or 8 (bits: 1 .. 8) chunks in the last slab; as the scalar offset takes no
// part in the range check, a lane whose chunk lies past Kb asks for an address that is out of range by itself.
struct ChunkCutLoader {
    uint32_t pvoff[8];
    uint32_t chunks = 0;     // 3 bits per piece: this lane's chunk of piece i
    int lw, last, keep;      // the last slab and how many chunks of it exist

    __device__ __forceinline__ ChunkCutLoader(int lw_, int lane, uint32_t pitch, int Kb, int T)
        : lw(lw_), last(T - 1), keep((Kb - (T - 1) * kStripRow) >> 4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            pvoff[i] = strip_piece_voff(lw * 8 + i, lane, pitch);
            chunks |= (uint32_t)strip_piece_chunk(lw * 8 + i, lane) << (3 * i);
        }
    }
    // piece i (a constant once unrolled) of slab u, of which the chunks below lim exist
    __device__ __forceinline__ void piece(__amdgpu_buffer_rsrc_t rsrc, char* stage, int u, int i, uint32_t lim) const {
        dma16(rsrc, stage + (lw * 8 + i) * kStripPiece, ((chunks >> (3 * i)) & 7u) >= lim ? kOOB : pvoff[i], u * kStripRow);
    }
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t rsrc, char* stage, int u) const {
        const uint32_t lim = u == last ? (uint32_t)keep : 8u;
#pragma unroll
        for (int i = 0; i < 8; ++i) piece(rsrc, stage, u, i, lim);
    }
};

// The block bytes of a slab for the lane half lhi, from the row's 8 bytes of that slab (one 8-byte load): byte s of the
// result is block 2 s + lhi, the scale a step s selects with op_sel.
__device__ __forceinline__ uint32_t fp4_pick_bytes(u32x2_t w, int lhi) {
    const int sh = 8 * lhi;
    return ((w[0] >> sh) & 0xffu) | (((w[0] >> (16 + sh)) & 0xffu) << 8) | (((w[1] >> sh) & 0xffu) << 16) |
           (((w[1] >> (16 + sh)) & 0xffu) << 24);
}

template <int S, int NB>
__device__ __forceinline__ void fp4_step(const StripLane& L, const char* stage, const uint32_t (&aexp)[NB], uint32_t bexp,
                                         f32x16_t (&acc)[NB]) {
    const int aoff = kStripSlab + L.lrow * kStripRow;
    const int ch = L.chunk(S * 2 + L.lhi);
    const i32x4_t b = *(const i32x4_t*)(stage + L.boff + ch);
    const i32x8_t b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const i32x4_t a = *(const i32x4_t*)(stage + aoff + j * 4096 + ch);
        const i32x8_t a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0};
        acc[j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a8, b8, acc[j], 4, 4, S, (int)aexp[j], S, (int)bexp);
    }
}

template <int NB>
__device__ __forceinline__ void fp4_slab_mma(const StripLane& L, const char* stage, uint32_t bexp, f32x16_t (&acc)[NB]) {
    const int eoff = kStripSlab + NB * 4096 + (L.lhi * NB * 32 + L.lrow) * 4;
    uint32_t aexp[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) aexp[j] = *(const uint32_t*)(stage + eoff + j * 128);
    fp4_step<0, NB>(L, stage, aexp, bexp, acc);   // k = 256 u + 64 s + 32 lhi + 0..31
    fp4_step<1, NB>(L, stage, aexp, bexp, acc);
    fp4_step<2, NB>(L, stage, aexp, bexp, acc);
    fp4_step<3, NB>(L, stage, aexp, bexp, acc);
}

// The same slab for a stage without block bytes in its query part (the list-major scan, whose query rows are gathered and
// have no image): the query rows' scale dwords come in registers, aexp[j] = the dword of query row 32 j + lrow for this
// lane half, picked like bexp.
template <int NB>
__device__ __forceinline__ void fp4_slab_mma(const StripLane& L, const char* stage, const uint32_t (&aexp)[NB], uint32_t bexp,
                                             f32x16_t (&acc)[NB]) {
    fp4_step<0, NB>(L, stage, aexp, bexp, acc);
    fp4_step<1, NB>(L, stage, aexp, bexp, acc);
    fp4_step<2, NB>(L, stage, aexp, bexp, acc);
    fp4_step<3, NB>(L, stage, aexp, bexp, acc);
}

// ---- sign bits ---------------------------------------------------------------------------------------------------------
// A 128-byte stage row of bits is 1024 k, eight times what a stage row of int8 query codes holds, so the two operands ride
// in two rings: the database ring keeps the 32 KB slabs above (ChunkCutLoader's pieces and cut by chunk: a row of bits is a
// multiple of 16 bytes, 1 .. 8 chunks in the last slab), the query ring holds index_i8.hip's 12 KB images of 128 k, eight
// of them to a database slab.  Sub-slab s of the walk is chunk s & 7 of slab s >> 3 on the database side.
__host__ __device__ inline int bin_row_bytes(int D) { return ((D + 127) >> 7) * 16; }   // bytes of a row of bits: D rounded up to 128
static constexpr int kBinSub = kQB * kStripRow;        // 12288: the query image of 128 k
static constexpr int kBinDbStages = 3, kBinQStages = 4;
static constexpr int kBinQOff = kBinDbStages * kStripSlab;
static constexpr int kBinLds = kBinQOff + kBinQStages * kBinSub;    // 147456 of 163840

// 16 bits -> 16 code bytes of 0 / 1: bit 4 d + e becomes byte e of dword d, the k order of the query bytes.  The four
// copies of a nibble at shifts 0, 7, 14, 21 do not overlap, and bits 0, 8, 16, 24 of their sum are its bits 0 .. 3.
__device__ __forceinline__ i32x4_t bin_widen(uint32_t h) {
    i32x4_t b;
#pragma unroll
    for (int d = 0; d < 4; ++d) b[d] = (int)((((h >> (4 * d)) & 0xfu) * 0x00204081u) & 0x01010101u);
    return b;
}

// One sub-slab: the lane's 16-byte chunk c of its row in the database slab `db` (128 bits, k = 128 s + 0 .. 127) against
// the query image `q` of the same k.  Step m takes the 16 bits of k = 32 m + 16 lhi + 0 .. 15, where the query operand is
// chunk 2 m + lhi of the query row, as in code_slab_mma.
template <int NB>
__device__ __forceinline__ void bin_sub_mma(const StripLane& L, const char* db, int c, const char* q, i32x16_t (&acc)[NB]) {
    const u32x4_t w = *(const u32x4_t*)(db + L.b(c));
    const int aoff = L.lrow * kStripRow, sh = 16 * L.lhi;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const i32x4_t b = bin_widen(w[m] >> sh);
        const int ch = L.chunk(m * 2 + L.lhi);
#pragma unroll
        for (int j = 0; j < NB; ++j)
            acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(*(const i32x4_t*)(q + aoff + j * 4096 + ch), b, acc[j], 0, 0, 0);
    }
}

}  // namespace dir

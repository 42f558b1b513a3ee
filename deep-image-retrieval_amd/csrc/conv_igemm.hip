// conv_igemm.hip — implicit-GEMM convolution for gfx950 (MFMA 32x32x16, 16-bit in / fp32 acc).
//
// Replaces every Conv2d + BatchNorm2d(eval) (+ residual add) (+ ReLU) of the reference trunk
// (dirtorch/nets/backbones/resnet.py:56-63,67-87,115-118,136-141) with one fused kernel family.
//
// GEMM view (per launch):   Y[m][n] = act( sum_k X[m][k] * Wt[n][k] + bias[n] (+ res[m][n]) )
//   m = (b, oh, ow) output pixel, n = output channel, k = (r, s, c) filter tap x input channel.
//   X is never materialised: for K-step (r, s, c0..c0+63) the 64-channel slice of input pixel
//   (oh*stride + r - pad, ow*stride + s - pad) is one contiguous 128-byte run of the NHWC tensor.
//   The stem (7x7 s2, Cin = 3) arrives as a 4x4 s1 convolution over the 2x2 space-to-depth image
//   (Cin = 16): one K-step = one filter row = four neighbouring pixels = the same 128-byte run.
//
// Data movement: HBM/L2 -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds) through two buffer
//   descriptors (activations, weights).  Per lane the 32-bit byte offset is computed ONCE; the
//   K-step advances through the instruction's scalar offset, so a 1x1 convolution spends no
//   VALU work per load.  Zero padding and the ragged last pixel tile use the descriptor's
//   bounds check: an out-of-range offset makes the hardware write zeros.
// LDS: an NST-slot ring of stages; a stage = X-tile [BM][64] + W-tile [BN][64], rows of 128 B whose
//   16-byte chunks are XOR-swizzled with ((row >> 1) & 7) so the MFMA fragment reads (ds_read_b128:
//   row = lane & 31, chunk = 2*ks + lane/32) are bank-conflict free.  The DMA destination is
//   lane-linear, so the swizzle is applied to the per-lane SOURCE chunk.  Waits are counted
//   (vmcnt = loads per stage x stages still in flight) and the barrier is the raw s_barrier, so
//   later stages stay in flight across it.
// MFMA operand roles are swapped (A = weights, B = pixels) so each lane ends up holding 4
//   consecutive output channels of one pixel.  Accumulators start at the folded-BN bias; the
//   epilogue stages them through LDS (fp32) and emits whole 16-byte runs (8 channels) with
//   residual add / ReLU / v_cvt_pk conversion fused.  Residual tiles are fetched before the K loop.
#include "dir_common.h"
#include "conv_device.h"
#include "conv_igemm.h"

#include <stdlib.h>
#include <string.h>
#include <algorithm>

namespace dir {

// SPLITK instantiations (a few small-tile variants) carry the split-K bookkeeping; the others compile
// exactly as if it did not exist - its extra scalar state costs 8-70 VGPRs in the big tiles.
// (The two-source form of rounds 2-3 - conv3 + the block's 1x1 downsample as one GEMM over [t2 ; x_s], one tile per
// workgroup - lives on the persistent ring since round 4: conv_persist.hip DUAL, bit-identical, 5-13 % faster.)
template <class DT, int BM, int BN, int WGM, int WGN, int NST, int BK, bool CIN16, bool SPLITK>
__global__ void __launch_bounds__(64 * WGM * WGN) conv_igemm_kernel(const ConvArgs a) {
    static_assert(NST >= 2 && NST <= 8, "ring depth");
    static_assert((BK == 64 || BK == 32) && (!CIN16 || BK == 64), "K-step");
    constexpr int RB = BK * 2;    // bytes per LDS row (one pixel / one output channel, BK channels)
    constexpr int CPR = BK / 8;   // 16-byte chunks per row
    constexpr int KS = BK / 16;   // MFMA k-substeps per stage
    constexpr int NT = 64 * WGM * WGN;
    constexpr int TM = BM / WGM / 32;  // pixel (B-operand) tiles per wave
    constexpr int TN = BN / WGN / 32;  // channel (A-operand) tiles per wave
    constexpr int NA = BM * CPR / NT;  // 16-byte X chunks per lane per stage
    constexpr int NB = BN * CPR / NT;  // 16-byte W chunks per lane per stage
    constexpr int LPS = NA + NB;       // DMA instructions per lane per stage
    static_assert(TM >= 1 && TN >= 1, "wave tile");
    static_assert(NA >= 1 && NB >= 1 && (BM * CPR) % NT == 0 && (BN * CPR) % NT == 0, "chunk split");
    static_assert((NT / CPR) % 16 == 0, "swizzle term must be constant per lane");
    constexpr int XS = BM * RB;  // bytes of the X tile of one stage
    constexpr int STAGE_BYTES = (BM + BN) * RB;
    constexpr int EROW = Staged<TN>::EROW;  // epilogue: one pixel row of TN*32 fp32 + pad
    typedef typename DT::frag_t frag_t;

    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WGN;
    const int wm = wave / WGN;
    const int lrow = lane & 31;
    const int lhi = lane >> 5;

    const int ntiles = a.tiles_m * a.tiles_n;
    const int wg = SPLITK ? xcd_remap(blockIdx.x % ntiles, ntiles) : xcd_remap(blockIdx.x, gridDim.x);
    const int kz = SPLITK ? blockIdx.x / ntiles : 0;  // split-K slice of this workgroup
    const int tile_n = wg % a.tiles_n;   // n fastest: blocks sharing an X tile run on one XCD
    const int tile_m = wg / a.tiles_n;

    const __amdgpu_buffer_rsrc_t rsrc_x = buffer_rsrc(a.x, a.x_bytes);
    const __amdgpu_buffer_rsrc_t rsrc_w = buffer_rsrc(a.w, a.w_bytes);

    // ---- per-lane source offsets (constant over the K loop) --------------------------------------
    // chunk slot `tid % CPR` of LDS row `tid / CPR (+ i*NT/CPR)` holds source chunk slot ^ swz(row):
    // swz = (row >> 1) & 7 for 128-byte rows, (row >> 2) & 3 for 64-byte rows (one 256-byte bank row
    // holds 2 resp. 4 LDS rows) - both reduce to bits of tid because NT/CPR is a multiple of 16.
    const int srcchunk = (tid & (CPR - 1)) ^ ((tid >> 4) & (CPR - 1));
    const bool one_tap = (a.R * a.S == 1);  // 1x1: no padding, K advances through the scalar offset
    int xbase[NA];       // byte offset of tap (0,0), channel chunk `srcchunk` (may be negative)
    uint32_t xmask[NA];  // bit per tap (stem: per filter row): tap inside the image and row valid
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int row = i * (NT / CPR) + tid / CPR;
        const int m = tile_m * BM + row;
        if (a.flat) {  // 1x1, stride 1: output pixel m reads input pixel m
            xbase[i] = (m * a.Cin + srcchunk * 8) * 2;
            xmask[i] = m < a.M ? 1u : 0u;
        } else {
            im2col_lane<CIN16>(a, m, srcchunk, xbase[i], xmask[i]);
        }
    }
    uint32_t xvoff[NA];  // 1x1 path: final voffset with the row mask folded in
#pragma unroll
    for (int i = 0; i < NA; ++i) xvoff[i] = (xmask[i] & 1u) ? (uint32_t)xbase[i] : kOOB;
    uint32_t wvoff[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int row = i * (NT / CPR) + tid / CPR;
        wvoff[i] = (uint32_t)(((tile_n * BN + row) * a.Ktot + srcchunk * 8) * 2);
    }
    // K-step t: filter tap `tap` (stem: filter row), byte offset `koff` of that tap/channel slice
    auto issue = [&](int t, int tap, int koff, char* stage) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            char* dst = stage + (i * NT + wave * 64) * 16;
            if (one_tap) {
                dma16(rsrc_x, dst, xvoff[i], koff);
            } else {
                const uint32_t v = ((xmask[i] >> tap) & 1u) ? (uint32_t)(xbase[i] + koff) : kOOB;
                dma16(rsrc_x, dst, v, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i)
            dma16(rsrc_w, stage + XS + (i * NT + wave * 64) * 16, wvoff[i], t * RB);
    };

    // ---- fragment read offsets -----------------------------------------------------------------
    const int lswz = BK == 64 ? ((lane >> 1) & 7) : ((lane >> 2) & 3);
    int loff[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) loff[ks] = lrow * RB + (((2 * ks + lhi) ^ lswz) << 4);
    const int xfrag = (wm * TM * 32) * RB;
    const int wfrag = XS + (wn * TN * 32) * RB;

    // ---- accumulators start at the bias of their 4 consecutive channels -----------------------
    f32x16_t acc[TN][TM];
    if (SPLITK)
        acc_init_zero(acc);   // split-K partial sums carry no bias
    else
        acc_init_bias(acc, a.bias + tile_n * BN + wn * TN * 32, lhi);

    auto compute = [&](const char* stage) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            frag_t wf[TN], xf[TM];
#pragma unroll
            for (int i = 0; i < TN; ++i)
                wf[i] = *(const frag_t*)(stage + wfrag + i * 32 * RB + loff[ks]);
#pragma unroll
            for (int j = 0; j < TM; ++j)
                xf[j] = *(const frag_t*)(stage + xfrag + j * 32 * RB + loff[ks]);
#pragma unroll
            for (int i = 0; i < TN; ++i)
#pragma unroll
                for (int j = 0; j < TM; ++j) acc[i][j] = DT::mfma32(wf[i], xf[j], acc[i][j]);
        }
    };

    // ---- residual tile fetched up front: its HBM latency hides under the whole K loop ----------
    constexpr int LPR = Staged<TN>::LPR, RPP = Staged<TN>::RPP, NPASS = Staged<TN>::NPASS;
    constexpr bool PRE_RES = (TM * NPASS <= 16); // 16 B per lane each: at most 64 VGPRs
    const int ecol = (lane % LPR) * 8;
    const int erow = lane / LPR;
    const int n_glob = tile_n * BN + wn * TN * 32 + ecol;
    const int m_epi = tile_m * BM + wm * TM * 32;
    u32x4_t rres[PRE_RES ? TM : 1][PRE_RES ? NPASS : 1];
    if (PRE_RES && !SPLITK && a.res) {
#pragma unroll
        for (int j = 0; j < TM; ++j)
#pragma unroll
            for (int pass = 0; pass < NPASS; ++pass) {
                const int m = m_epi + j * 32 + pass * RPP + erow;
                const int mc = m < a.M ? m : 0;  // clamped rows are never stored
                rres[PRE_RES ? j : 0][PRE_RES ? pass : 0] =
                    gload16(a.res + ((size_t)mc * a.Cout + n_glob));
            }
    }

    // ---- K loop: NST-slot ring fed by LDS-DMA ----------------------------------------------------
    // Stages t+1 .. t+NST-1 stay in flight while stage t is consumed.  One barrier per K-step:
    // passing it means (a) stage t has landed for every wave (each waited on its own counted vmcnt
    // first), (b) every wave has finished reading slot (t-1) % NST, the slot refilled right after.
    const int cpb = CIN16 ? 1 : (a.Cin / BK);  // K-steps per filter tap
    const int t_begin = SPLITK ? (int)((long)a.T * kz / a.ksplit) : 0;
    const int T = SPLITK ? (int)((long)a.T * (kz + 1) / a.ksplit) - t_begin : a.T;  // this workgroup's K-steps
    // K order: channel slice outermost, filter taps innermost.  Consecutive K-steps of a 3x3 conv
    // then read the SAME 64-channel slice of the input at pixel-shifted positions, so eight of the
    // nine tap reads hit the XCD's L2 (a tap-major order spaced those re-reads Cin/64 steps apart,
    // 32 CUs x that footprint overflowed the 4 MB L2 and the 3x3 layers fetched their input ~3x
    // from the fabric - profiles/r01_bench_b32_hbm_pmc.json history).  The stem (CIN16) has one
    // K-step per filter row and keeps row order.
    KWalker<BK, CIN16> kw;                     // the step being ISSUED
    if (SPLITK && t_begin > 0) kw.seek(a, t_begin);
    int issued = 0;
#pragma unroll
    for (int p = 0; p < NST - 1; ++p) {
        if (p < T) {
            issue(kw.wstep(cpb), kw.tap, kw.koff(a), smem + p * STAGE_BYTES);
            kw.advance(a);
            ++issued;
        }
    }
    int slot_c = 0;        // slot holding stage t
    int slot_i = issued;   // slot the next issue goes to
    if (slot_i == NST) slot_i = 0;
    for (int t = 0; t < T; ++t) {
        const int ahead = issued - 1 - t;  // stages issued beyond t: 0 .. NST-2
        // (deep rings, round 6: the small-tile variants of the small-map regime keep up to six stages in flight)
        static_assert((NST - 2) * LPS <= 63, "vmcnt immediate");
        if (NST >= 8 && ahead >= 6) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST >= 8 ? 6 * LPS : 0) : "memory");
        } else if (NST >= 7 && ahead >= 5) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST >= 7 ? 5 * LPS : 0) : "memory");
        } else if (NST >= 6 && ahead >= 4) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST >= 6 ? 4 * LPS : 0) : "memory");
        } else if (NST >= 5 && ahead >= 3) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NST >= 5 ? 3 * LPS : 0) : "memory");
        } else if (NST >= 4 && ahead >= 2) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * LPS) : "memory");
        } else if (NST >= 3 && ahead == 1) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(LPS) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        ring_barrier();
        if (issued < T) {
#ifndef DIR_EXP_NO_FILL     // experiment builds (scripts/exp_abl.sh conv_igemm DIR_EXP_NO_FILL 1): MFMA + fragment reads alone
            issue(kw.wstep(cpb), kw.tap, kw.koff(a), smem + slot_i * STAGE_BYTES);
#endif
            kw.advance(a);
            ++issued;
            if (++slot_i == NST) slot_i = 0;
        }
#ifndef DIR_EXP_FILL_ONLY   // experiment builds: the LDS-DMA ring alone
        compute(smem + slot_c * STAGE_BYTES);
#endif
        if (++slot_c == NST) slot_c = 0;
    }
    __syncthreads();  // all fragment reads done before the epilogue reuses the ring
    Ovf<DT> ovf;

    // ---- epilogue: acc -> LDS (fp32, pixel-major) -> residual / ReLU / convert -> 16-byte stores --
    // (conv_device.h's epilogue_strip, written out: through the helper the 256x128 _k32 forms took 130 VGPRs instead of 128 - one
    // wave per SIMD less - and 256x256_w4x4 spilled 8 registers)
    char* ebase = smem + wave * (32 * EROW);
#pragma unroll
    for (int j = 0; j < TM; ++j) {
#pragma unroll
        for (int i = 0; i < TN; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4_t v = {acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2],
                             acc[i][j][4 * g + 3]};
                const int n_local = i * 32 + 8 * g + 4 * lhi;
                *(f32x4_t*)(ebase + lrow * EROW + n_local * 4) = v;
            }
        wave_lds_sync();
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            const int mrow = pass * RPP + erow;
            const f32x4_t f0 = *(const f32x4_t*)(ebase + mrow * EROW + ecol * 4);
            const f32x4_t f1 = *(const f32x4_t*)(ebase + mrow * EROW + ecol * 4 + 16);
            const int m = m_epi + j * 32 + mrow;
            if (SPLITK && m < a.M) {   // raw fp32 partial sums; conv_splitk_finalize does the rest
                float* po = a.partial + ((size_t)kz * a.M + m) * a.Cout + n_glob;
                *(DIR_GLOBAL f32x4_t*)po = f0;
                *(DIR_GLOBAL f32x4_t*)(po + 4) = f1;
            } else if (!SPLITK && m < a.M) {
                float v[8] = {f0[0], f0[1], f0[2], f0[3], f1[0], f1[1], f1[2], f1[3]};
                const size_t o = (size_t)m * a.Cout + n_glob;
                if (a.res) add_res8<DT>(v, PRE_RES ? rres[PRE_RES ? j : 0][PRE_RES ? pass : 0] : gload16(a.res + o));
                if (a.relu) relu8(v);
                const u32x4_t ov = pack8<DT>(v);
                gstore16(a.y + o, ov);
                ovf.see(ov);
            }
        }
        wave_lds_sync();
    }
    ovf.flush(a.ovf);
}

// ---- variant table ----------------------------------------------------------------------------
template <class DT, int BM, int BN, int WGM, int WGN, int NST, int BK, bool CIN16, bool SPLITK = false>
static hipError_t launch_variant(const ConvArgs& a, hipStream_t stream) {
    constexpr int NT = 64 * WGM * WGN;
    constexpr int TN = BN / WGN / 32;
    constexpr int EROW = Staged<TN>::EROW;
    constexpr int STAGE_BYTES = (BM + BN) * BK * 2;
    constexpr int EPI_BYTES = (NT / 64) * 32 * EROW;
    constexpr int LDS = (NST * STAGE_BYTES > EPI_BYTES) ? NST * STAGE_BYTES : EPI_BYTES;
    static_assert(LDS <= 160 * 1024, "LDS budget");
    auto kern = conv_igemm_kernel<DT, BM, BN, WGM, WGN, NST, BK, CIN16, SPLITK>;
    static std::atomic<uint64_t> attr_done{0};
    if (hipError_t e = ensure_dynamic_lds((const void*)kern, LDS, attr_done); e != hipSuccess) return e;
    ConvArgs b = a;
    b.T = a.Ktot / BK;
    b.tiles_m = ceil_div(a.M, BM);
    b.tiles_n = a.Cout / BN;
    conv_fill_extents(b);
    b.flat = (a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0 && a.H == a.OH && a.W == a.OW);
    // a short K loop never touches the far slots of the ring: ask for less LDS, more residency
    const int used = (b.T < NST ? b.T : NST) * STAGE_BYTES;
    const int lds = used > EPI_BYTES ? used : EPI_BYTES;
    const int nz = SPLITK ? a.ksplit : 1;
    hipLaunchKernelGGL(kern, dim3(b.tiles_m * b.tiles_n * nz), dim3(NT), lds, stream, b);
    return hipGetLastError();
}

// What an implicit-GEMM row launches: the instantiation for the dtype, or - where the row has them - its Cin == 16 form (the
// space-to-depth stem) or its split-K form (ConvArgs::ksplit > 1; conv_launch refuses that on a row without one).
// (The forms are named in the order plain, Cin == 16, split-K: the order their kernels are instantiated and emitted in.)
template <int BM, int BN, int WGM, int WGN, int NST, int BK, bool HAS16, bool HASSK>
static hipError_t launch_igemm(const ConvArgs& a, int dtype, hipStream_t stream) {
    const bool bf = dtype == DIR_BF16;
    hipError_t (*fn)(const ConvArgs&, hipStream_t) = bf ? launch_variant<BF16, BM, BN, WGM, WGN, NST, BK, false>
                                                        : launch_variant<FP16, BM, BN, WGM, WGN, NST, BK, false>;
    if constexpr (HAS16)
        if (a.Cin == 16) fn = bf ? launch_variant<BF16, BM, BN, WGM, WGN, NST, BK, true> : launch_variant<FP16, BM, BN, WGM, WGN, NST, BK, true>;
    if constexpr (HASSK)
        if (a.ksplit > 1) fn = bf ? launch_variant<BF16, BM, BN, WGM, WGN, NST, BK, false, true> : launch_variant<FP16, BM, BN, WGM, WGN, NST, BK, false, true>;
    return fn(a, stream);
}
template <int BN, bool HAS16>
static bool igemm_admissible(const ConvArgs& a) {
    return a.Cout % BN == 0 && (HAS16 || a.Cin != 16);
}
// conv_patch.hip's one-tile-of-Cout kernel: a row per channel count
template <int C>
static bool patch3x3_admissible(const ConvArgs& a) {
    return a.Cout == C && conv_patch3x3_admissible(a);
}

#define DIR_IGEMM_ROW(BM, BN, WGM, WGN, NST, BK, HAS16, HASSK, NAME)                         \
    {NAME, BM, BN, 64 * WGM * WGN, NST, BK, igemm_admissible<BN, HAS16>,                     \
     launch_igemm<BM, BN, WGM, WGN, NST, BK, HAS16, HASSK>, HASSK, nullptr, nullptr}
#define DIR_VARIANT(BM, BN, WGM, WGN, NST, BK, NAME) DIR_IGEMM_ROW(BM, BN, WGM, WGN, NST, BK, false, false, NAME)
// ... plus the split-K instantiation (small-M layers)
#define DIR_VARIANT_SK(BM, BN, WGM, WGN, NST, BK, NAME) DIR_IGEMM_ROW(BM, BN, WGM, WGN, NST, BK, false, true, NAME)
// BN == 64 variants also carry the Cin == 16 (space-to-depth stem) instantiation.
#define DIR_VARIANT16(BM, BN, WGM, WGN, NST, NAME) DIR_IGEMM_ROW(BM, BN, WGM, WGN, NST, 64, true, false, NAME)
// a row bound to another source's kernel: {admissible, launch} and, where it has a two-source form, the same pair for it
#define DIR_ROW(NAME, BM, BN, THREADS, NST, BK, ADM, LAUNCH) {NAME, BM, BN, THREADS, NST, BK, ADM, LAUNCH, false, nullptr, nullptr}
#define DIR_ROW_DUAL(NAME, BM, BN, THREADS, NST, BK, ADM, LAUNCH, ADM2, LAUNCH2) {NAME, BM, BN, THREADS, NST, BK, ADM, LAUNCH, false, ADM2, LAUNCH2}

// name = <pixels>x<channels>_w<waves m>x<waves n>[_s<ring depth>][_k<K-step>]
static const ConvVariant kVariants[] = {
    DIR_VARIANT_SK(128, 128, 2, 2, 2, 64, "128x128_w2x2"),
    DIR_VARIANT16(128, 64, 2, 2, 2, "128x64_w2x2"),
    DIR_VARIANT16(256, 64, 4, 1, 2, "256x64_w4x1"),
    DIR_VARIANT(256, 128, 4, 2, 2, 64, "256x128_w4x2"),
    DIR_VARIANT(128, 256, 2, 4, 2, 64, "128x256_w2x4"),
    DIR_VARIANT(256, 256, 4, 2, 2, 64, "256x256_w4x2"),
    DIR_VARIANT_SK(64, 128, 2, 2, 2, 64, "64x128_w2x2"),
    DIR_VARIANT16(64, 64, 2, 1, 2, "64x64_w2x1"),
    DIR_VARIANT(64, 128, 2, 2, 4, 64, "64x128_w2x2_s4"),
    DIR_VARIANT(128, 128, 2, 2, 3, 64, "128x128_w2x2_s3"),
    DIR_VARIANT16(128, 64, 2, 2, 4, "128x64_w2x2_s4"),
    DIR_VARIANT(256, 128, 4, 2, 3, 64, "256x128_w4x2_s3"),
    DIR_VARIANT(128, 256, 2, 4, 3, 64, "128x256_w2x4_s3"),
    DIR_VARIANT16(256, 64, 4, 1, 3, "256x64_w4x1_s3"),
    DIR_VARIANT(256, 256, 4, 2, 4, 32, "256x256_w4x2_s4_k32"),
    DIR_VARIANT(256, 256, 4, 2, 3, 32, "256x256_w4x2_s3_k32"),
    DIR_VARIANT(256, 128, 4, 2, 4, 32, "256x128_w4x2_s4_k32"),
    DIR_VARIANT(128, 128, 2, 2, 4, 32, "128x128_w2x2_s4_k32"),
    // 72 KB of LDS and <= 128 VGPRs: two 512-thread workgroups share a CU, so one's epilogue
    // overlaps the other's K loop (the memory-bound 1x1 convs of layer3/4)
    DIR_VARIANT(256, 128, 4, 2, 3, 32, "256x128_w4x2_s3_k32"),
    DIR_VARIANT(128, 256, 2, 4, 3, 32, "128x256_w2x4_s3_k32"),
    DIR_VARIANT(128, 256, 2, 2, 3, 32, "128x256_w2x2_s3_k32"),   // two 256-thread workgroups per CU
    DIR_VARIANT(128, 128, 2, 2, 3, 32, "128x128_w2x2_s3_k32"),   // 48 KB: three workgroups per CU
    // 16 waves of 64x64 on one CU (128 VGPRs): more fragment reads in flight under the matrix
    // pipe - the 3x3 convs of layer3/4
    DIR_VARIANT(256, 256, 4, 4, 2, 64, "256x256_w4x4"),
    // the small-map regime (batch 1 / 224^2 buckets: 1 000 - 13 000 pixels per layer): 64x64 tiles give every CU one even at
    // 4 096 pixels x 256 channels.  _s4 (64 KB: two workgroups per CU - what forwards overlapping on several streams need) is the
    // picker's choice: batch 1 at 1024^2 768 -> 799 img/s on one stream, 1 320 -> 1 366 on four; _s8 (six 16 KB stages in flight,
    // 128 KB) is 1 % better on one stream and 20 % worse on four (806 / 1 075, gpurun_out/r6smallab2) - a tuner candidate
    DIR_VARIANT_SK(64, 64, 2, 2, 8, 64, "64x64_w2x2_s8"),
    DIR_VARIANT_SK(64, 64, 2, 2, 4, 64, "64x64_w2x2_s4"),
    // 3x3 stride-1 from an LDS-resident input patch (conv_patch.hip): 8x32 pixels x all channels
    DIR_ROW("256x64_patch3x3", 256, 64, 256, 3, 64, patch3x3_admissible<64>, conv_patch3x3_launch),
    DIR_ROW("256x128_patch3x3", 256, 128, 512, 3, 64, patch3x3_admissible<128>, conv_patch3x3_launch),
    // ... 64 -> 64 channels without a residual: the whole filter resident in LDS, double-buffered patches, loader waves
    // fetch while consumer waves multiply (conv_patchlc.hip)
    DIR_ROW("256x64_patchlc3x3", 256, 64, 512, 2, 64, conv_patch64_lc_admissible, conv_patch64_lc_launch),
    // ... for the wide 3x3 layers (256 / 512 channels): the patch one 64-channel plane at a time, Cout tiled by 256
    DIR_ROW("256x256_patch3x3s", 256, 256, 512, 2, 64, conv_patch3x3s_admissible, conv_patch3x3s_launch),
    // ... 512 pixels x 128 channels per workgroup, 32-channel planes double-buffered, one filter row per weight stage
    DIR_ROW("512x128_patch3x3w", 512, 128, 512, 3, 32, conv_patch3x3w_admissible, conv_patch3x3w_launch),
    // 3x3 STRIDE 2 (conv2 of the first block of layers 2-4): persistent, 8 x 32 output pixels x 128 channels from a 17 x 65 patch,
    // 32-channel planes double-buffered with even / odd input columns apart, weights straight into registers (conv_patchs2.hip)
    DIR_ROW("256x128_patchs2", 256, 128, 768, 2, 32, conv_patch3x3s2_admissible, conv_patch3x3s2_launch),
    // persistent workgroups, next tile's first K-stage issued before the epilogue (conv_persist.hip)
    DIR_ROW("256x256_persist1x1", 256, 256, 512, 2, 64, conv1x1_persist_admissible, conv1x1_persist_launch),
    // the same with three K-steps of the pixel operand in the ring (HBM requests in flight: 32 -> 64+ KB per CU)
    // ... and its two-source form (conv3 + downsample of the first block of layers 2-4)
    DIR_ROW_DUAL("256x256_persist1x1_x3", 256, 256, 512, 3, 64, conv1x1_persist_x3_admissible, conv1x1_persist_x3_launch,
                 conv1x1_persist_dual_admissible, conv1x1_persist_dual_launch),
    // persistent 128x256 tile, loader waves feed ONE three-slot K ring over all the tiles of a workgroup, consumer waves
    // multiply; 1x1 convs without a residual (conv_ring.hip)
#ifdef DIR_EXPERIMENTS   // (csrc/build.sh with DIR_EXPERIMENTS=1: ties conv_persist.hip inside the network, not a default build's kernel)
    DIR_ROW("128x256_ring1x1", 128, 256, 512, 3, 64, conv1x1_ring_admissible, conv1x1_ring_launch),
#endif
    // persistent, 64 output channels x K <= 256 per wave held in VGPRs, only pixels stream (conv_wreg.hip)
    DIR_ROW("64x512_wreg1x1", 64, 512, 512, 2, 64, conv1x1_wreg_admissible, conv1x1_wreg_launch),
    // small maps (batch 1 at native size): 64 x 64 tiles, four consumer + four loader waves that meet on LDS counters, no workgroup
    // barrier in the loop (conv_small.hip); _s4 = 64 KB (two workgroups per CU), _s8 = 128 KB
    DIR_ROW("64x64_small_s8", 64, 64, 512, 8, 64, conv_small_admissible, conv_small_s8_launch),
    DIR_ROW("64x64_small_s4", 64, 64, 512, 4, 64, conv_small_admissible, conv_small_s4_launch),
    DIR_ROW("64x64_small_s4k2", 64, 64, 512, 4, 64, conv_small_k2_admissible, conv_small_s4k2_launch),   // 4 slots x 2 K-steps per stage
    // the deep-X ring with loader / consumer wave roles (eight consumers, four loaders): 1x1 without a residual, and its two-source form
    DIR_ROW_DUAL("256x256_lc1x1", 256, 256, 768, 3, 64, conv1x1_lc_plain_admissible, conv1x1_lc_launch,
                 conv1x1_lc_admissible, conv1x1_lc_dual_launch),
    // the two-source GEMM of layer2's first block (K = 128 + 256) with 32 output channels x 384 inputs per wave held in VGPRs,
    // 256 channels per workgroup (conv_wregd.hip); a two-source-only row: never admissible for a plain conv
    DIR_ROW_DUAL("64x256_wregd1x1", 64, 256, 512, 2, 64, nullptr, nullptr, conv1x1_wregd_admissible, conv1x1_wregd_launch),
};
static constexpr int kNumVariants = sizeof(kVariants) / sizeof(kVariants[0]);

int conv_variant_count() { return kNumVariants; }
const ConvVariant& conv_variant(int i) { return kVariants[i]; }

bool conv_variant_admissible(int v, const ConvArgs& a) {
    return v >= 0 && v < kNumVariants && kVariants[v].admissible != nullptr && kVariants[v].admissible(a);
}
// (conv_pick_variant, conv_pick_dual_variant and conv_splitk_factor - which row a shape takes - are conv_pick.hip's)

// ---- split-K ---------------------------------------------------------------------------------------
// y = act(sum_z partial[z] + bias (+ res)): the z order is fixed, so the result does not depend on
// which workgroup finished first.  8 channels per lane.
template <class DT>
__global__ void conv_splitk_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ bias,
                                            const uint16_t* res, uint16_t* y,   // (no __restrict__: in-place identity blocks pass res == y)
                                            long total8, int Cout, long MC, int ksplit, int relu, int* ovf_flag) {
    const long i8 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i8 >= total8) return;
    const long o = i8 * 8;
    const int n = (int)(o % Cout);
    float v[8];
    const f32x4_t b0 = *(const DIR_GLOBAL f32x4_t*)(bias + n), b1 = *(const DIR_GLOBAL f32x4_t*)(bias + n + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = b0[e], v[4 + e] = b1[e];
    for (int z = 0; z < ksplit; ++z) {
        const float* p = partial + (size_t)z * MC + o;
        const f32x4_t p0 = *(const DIR_GLOBAL f32x4_t*)p, p1 = *(const DIR_GLOBAL f32x4_t*)(p + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += p0[e], v[4 + e] += p1[e];
    }
    if (res) add_res8<DT>(v, gload16(res + o));
    if (relu) relu8(v);
    const u32x4_t ov = pack8<DT>(v);
    gstore16(y + o, ov);
    Ovf<DT> ovf;
    ovf.see(ov);
    ovf.flush(ovf_flag);
}

int conv_launch(const ConvArgs& a, int dtype, int variant, hipStream_t stream) {
    if (a.Cout % 64 != 0) return fail(DIR_ERR_INVALID, "conv: Cout must be a multiple of 64");
    const bool cin16 = (a.Cin == 16);
    if (cin16) {
        if (a.R != 4 || a.S != 4 || a.stride != 1)
            return fail(DIR_ERR_INVALID, "conv: Cin == 16 is only the 4x4 s1 space-to-depth stem");
    } else if (a.Cin % 64 != 0) {
        return fail(DIR_ERR_INVALID, "conv: Cin must be a multiple of 64 (or 16 for the stem)");
    }
    if (a.R > 4 || a.S > 4) return fail(DIR_ERR_INVALID, "conv: filter larger than 4x4");
    if ((long)a.B * a.H * a.W * a.Cin >= (1L << 30) || (long)a.M * a.Cout >= (1L << 30) ||
        (long)a.Cout * a.Ktot >= (1L << 30))
        return fail(DIR_ERR_INVALID, "conv: tensor exceeds 2^31 bytes; lower the batch");
    if (((uintptr_t)a.x & 15) || ((uintptr_t)a.w & 15) || ((uintptr_t)a.y & 15) ||
        ((uintptr_t)a.res & 15) || ((uintptr_t)a.bias & 15))
        return fail(DIR_ERR_INVALID, "conv: tensors must be 16-byte aligned");
    if (dtype != DIR_BF16 && dtype != DIR_FP16) return fail(DIR_ERR_INVALID, "conv: bad dtype");
    if (a.x2) {   // two-source K: conv3 + downsample in one GEMM
        if (variant < 0) variant = conv_pick_dual_variant(a);
        if (variant < 0 || variant >= kNumVariants || kVariants[variant].launch_dual == nullptr ||
            !kVariants[variant].admissible_dual(a) || a.R != 1 || a.S != 1 || a.stride != 1 || a.res || a.ksplit > 1 ||
            a.Cin2 % 64 != 0 || a.Ktot != a.Cin + a.Cin2 || ((uintptr_t)a.x2 & 15) ||
            (long)a.B * a.H2 * a.W2 * a.Cin2 >= (1L << 30))
            return fail(DIR_ERR_INVALID, "conv: no two-source form for this shape / variant");
        hipError_t e = kVariants[variant].launch_dual(a, dtype, stream);
        if (e != hipSuccess)
            return fail(DIR_ERR_HIP, std::string("conv launch ") + kVariants[variant].name + "/dual: " + hipGetErrorString(e));
        return DIR_OK;
    }
    if (variant < 0) variant = conv_pick_variant(a);
    if (!conv_variant_admissible(variant, a))
        return fail(DIR_ERR_INVALID, "conv: variant not admissible for this shape");
    const ConvVariant& cv = kVariants[variant];
    if (a.ksplit > 1) {
        if (!cv.has_splitk || cin16)
            return fail(DIR_ERR_INVALID, "conv: this variant has no split-K form");
        if (!a.partial || ((uintptr_t)a.partial & 15))
            return fail(DIR_ERR_INVALID, "conv: split-K needs a 16-byte aligned fp32 scratch buffer");
        if (a.ksplit > a.Ktot / cv.BK) return fail(DIR_ERR_INVALID, "conv: more K slices than K-steps");
    }
    hipError_t e = cv.launch(a, dtype, stream);
    if (e != hipSuccess)
        return fail(DIR_ERR_HIP, std::string("conv launch ") + cv.name + ": " + hipGetErrorString(e));
    if (a.ksplit > 1) {
        const long MC = (long)a.M * a.Cout, total8 = MC / 8;
        const dim3 grid((unsigned)((total8 + 255) / 256));
        if (dtype == DIR_BF16)
            hipLaunchKernelGGL(conv_splitk_finalize_kernel<BF16>, grid, dim3(256), 0, stream, a.partial, a.bias,
                               a.res, a.y, total8, a.Cout, MC, a.ksplit, a.relu, a.ovf);
        else
            hipLaunchKernelGGL(conv_splitk_finalize_kernel<FP16>, grid, dim3(256), 0, stream, a.partial, a.bias,
                               a.res, a.y, total8, a.Cout, MC, a.ksplit, a.relu, a.ovf);
        e = hipGetLastError();
        if (e != hipSuccess) return fail(DIR_ERR_HIP, std::string("conv split-K finalize: ") + hipGetErrorString(e));
    }
    return DIR_OK;
}

// ---- naive checker kernel ------------------------------------------------------------------------
template <class DT>
__global__ void conv_naive_kernel(const ConvArgs a) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)a.M * a.Cout) return;
    const int n = (int)(idx % a.Cout);
    const int m = (int)(idx / a.Cout);
    const int OHW = a.OH * a.OW;
    const int b = m / OHW, rem = m - b * OHW, oh = rem / a.OW, ow = rem - oh * a.OW;
    float acc = 0.f;
    for (int r = 0; r < a.R; ++r) {
        const int ih = oh * a.stride - a.pad + r;
        if ((unsigned)ih >= (unsigned)a.H) continue;
        for (int s = 0; s < a.S; ++s) {
            const int iw = ow * a.stride - a.pad + s;
            if ((unsigned)iw >= (unsigned)a.W) continue;
            const uint16_t* xp = a.x + ((size_t)(b * a.H + ih) * a.W + iw) * a.Cin;
            const uint16_t* wp = a.w + (size_t)n * a.Ktot + (r * a.S + s) * a.Cin;
            for (int c = 0; c < a.Cin; ++c) acc = fmaf(DT::to_f32(xp[c]), DT::to_f32(wp[c]), acc);
        }
    }
    float v = acc + a.bias[n];
    if (a.res) v += DT::to_f32(a.res[(size_t)m * a.Cout + n]);
    if (a.relu) v = fmaxf(v, 0.f);
    a.y[(size_t)m * a.Cout + n] = DT::from_f32(v);
}

int conv_launch_naive(const ConvArgs& a, int dtype, hipStream_t stream) {
    const long total = (long)a.M * a.Cout;
    const int threads = 256;
    const long blocks = (total + threads - 1) / threads;
    if (blocks >= (1L << 31)) return fail(DIR_ERR_INVALID, "naive conv: too many blocks");
    if (dtype == DIR_BF16)
        hipLaunchKernelGGL(conv_naive_kernel<BF16>, dim3((unsigned)blocks), dim3(threads), 0, stream, a);
    else
        hipLaunchKernelGGL(conv_naive_kernel<FP16>, dim3((unsigned)blocks), dim3(threads), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(DIR_ERR_HIP, std::string("naive conv: ") + hipGetErrorString(e));
    return DIR_OK;
}

}  // namespace dir

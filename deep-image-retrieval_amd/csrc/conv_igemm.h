// conv_igemm.h — host-side contract of the implicit-GEMM convolution family (conv_igemm.hip).
#pragma once
#include "dir_common.h"

namespace dir {

struct ConvArgs {
    const uint16_t* x;     // NHWC [B,H,W,Cin]
    const uint16_t* w;     // [Cout][R][S][Cin]
    const float* bias;     // [Cout]  (folded BatchNorm shift)
    const uint16_t* res;   // NHWC [B,OH,OW,Cout] or nullptr
    uint16_t* y;           // NHWC [B,OH,OW,Cout]
    int B, H, W, Cin, OH, OW, Cout;
    int R, S, stride, pad, relu;
    int M;     // B*OH*OW
    int Ktot;  // R*S*Cin
    int T;     // Ktot / 64
    // split-K (small M: too few output tiles to fill the chip).  ksplit > 1: workgroup (tile, z)
    // accumulates K-steps [z*T'/ksplit, (z+1)*T'/ksplit) and stores raw fp32 sums to
    // partial[z][M][Cout]; conv_splitk_finalize adds them in z order with bias / residual / ReLU.
    int ksplit;      // 0 or 1 = off
    float* partial;
    // fused bottleneck seam (conv_c3c1.hip): the NEXT block's conv1 applied to this conv's output tile
    const uint16_t* w2;    // [Cout2][Cout]
    const float* bias2;    // [Cout2]
    uint16_t* y2;          // NHWC [B,OH,OW,Cout2]
    int Cout2, relu2;
    // ... and, for the first block of a stage, the block input as a second K source (the downsample conv
    // folded into this GEMM): x2 [M][Cin2], its weights appended to w along K, its bias added to bias
    const uint16_t* x2;
    int Cin2;
    // ... or (two-source GEMM, conv_persist.hip DUAL) any 1x1 downsample: x2 is NHWC [B,H2,W2,Cin2], output
    // pixel (b, oh, ow) reads x2 pixel (b, oh*stride2, ow*stride2)
    int H2, W2, stride2;
    uint32_t x2_bytes;
    int* ovf;              // fp16 overflow word (dir_common.h Ovf), or nullptr
    // paired-fp16 form (conv_pair.hip, DIR_FP16P): every operand is a PAIR of fp16 planes, value = hi + lo with
    // lo = fp16(v - hi) (~22 significant bits); x / w / res / y above are the hi planes, these the lo planes of the
    // same layout.  w_lo is required there; x_lo / res_lo / y_lo may be null (single-plane operand / output).
    const uint16_t* x_lo;
    const uint16_t* x2_lo;   // ... and of the second K source (x2) in the two-source form
    const uint16_t* w_lo;
    const uint16_t* w_pw;    // conv_patchw.hip (loader / consumer form): w as its LDS stage images (conv_patch3x3w_pack), or null (gathered from w)
    const uint16_t* w_s2;    // conv_patchs2.hip: w in fragment order (conv_patch3x3s2_pack), or null (the launcher packs into scratch)
    const uint16_t* w2_lo;   // the fused seam (conv_c3c1.hip, WP1): lo plane of the following conv1's weights
    const uint16_t* res_lo;
    uint16_t* y_lo;
    // filled by the launcher
    int tiles_m, tiles_n;
    uint32_t x_bytes, w_bytes;               // buffer-descriptor extents (bounds-checked DMA)
    int rev_m;                               // persistent 1x1: walk the pixel tiles from the LAST one (read what the
                                             // producer wrote most recently first: it is still in the 256 MB Infinity Cache)
    int no_xcd_map;                          // persistent kernels: 1 = tiles follow blockIdx (A/B; default 0 = XCD-aware)
    int flat;                                // 1x1, stride 1, no padding: pixel m reads pixel m
    uint32_t div_ohw_mul, div_ohw_shr;       // exact n / (OH*OW) and n / OW for n < 2^31
    uint32_t div_ow_mul, div_ow_shr;
    // the fused seam at a stage exit (conv_c3c1.hip): s > 1 = y receives only the pixels with row % s == 0 && col % s == 0 of
    // each image, at their places in the full-resolution layout - all that the next stage's 1x1 stride-s downsample reads of
    // it; every other element of y is left as it was.  0 or 1 = every pixel is stored.  (y2 is complete either way.)
    int y_keep_stride;
    uint32_t div_keep_mul, div_keep_shr;     // filled by the launcher: exact n / y_keep_stride
};

// ---- launcher prologue (host half of conv_device.h) ----------------------------------------------------------------------
// Constants of fast_div (conv_device.h): q = umulhi(n, mul) >> shr is exact for 0 <= n < 2^31
// (mul = ceil(2^(31+l) / d), l = ceil(log2 d)); mul == 0 encodes division by 1.
inline void fastdiv_init(uint32_t d, uint32_t& mul, uint32_t& shr) {
    if (d <= 1) {
        mul = 0;
        shr = 0;
        return;
    }
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    mul = (uint32_t)(((1ull << (31 + l)) + d - 1) / d);
    shr = l - 1;
}

// What every launcher derives from the shape alone: the buffer-descriptor extents of the NHWC input(s) and the filter, and
// the divisors that turn an output pixel index into (b, oh, ow).
inline void conv_fill_extents(ConvArgs& b) {
    b.x_bytes = (uint32_t)((size_t)b.B * b.H * b.W * b.Cin * 2);
    b.w_bytes = (uint32_t)((size_t)b.Cout * b.Ktot * 2);
    if (b.x2) b.x2_bytes = (uint32_t)((size_t)b.B * b.H2 * b.W2 * b.Cin2 * 2);
    fastdiv_init((uint32_t)(b.OH * b.OW), b.div_ohw_mul, b.div_ohw_shr);
    fastdiv_init((uint32_t)b.OW, b.div_ow_mul, b.div_ow_shr);
}

// ---- how a geometry and its tensors become a ConvArgs ---------------------------------------------------------------------
// What a layer and an input shape fix about one convolution.
struct ConvGeom {
    int B, H, W, Cin, Cout, R, S, stride, pad, OH, OW, relu;
};
// Zero-fills `a` (padding included: every optional pointer null, split-K off), fills the geometry and the primary tensors
// and derives M = B*OH*OW and Ktot = R*S*Cin.  A template because the strict path's ConvF32Args (conv_f32.h) is filled the same way.
template <class Args, class Elem>
inline void conv_geom_fill(Args& a, const ConvGeom& g, const Elem* x, const Elem* w, const float* bias, const Elem* res, Elem* y) {
    memset(&a, 0, sizeof(a));
    a.x = x;
    a.w = w;
    a.bias = bias;
    a.res = res;
    a.y = y;
    a.B = g.B;
    a.H = g.H;
    a.W = g.W;
    a.Cin = g.Cin;
    a.OH = g.OH;
    a.OW = g.OW;
    a.Cout = g.Cout;
    a.R = g.R;
    a.S = g.S;
    a.stride = g.stride;
    a.pad = g.pad;
    a.relu = g.relu;
    a.M = g.B * g.OH * g.OW;
    a.Ktot = g.R * g.S * g.Cin;
}
// ... and for ConvArgs T as well.  The two-source, seam and paired fields are the caller's, below or by plain assignment.
inline void conv_args_init(ConvArgs& a, const ConvGeom& g, const uint16_t* x, const uint16_t* w, const float* bias,
                           const uint16_t* res, uint16_t* y) {
    conv_geom_fill(a, g, x, w, bias, res, y);
    a.T = a.Ktot / 64;
}
// A second K source appended to a 1x1 conv's own (conv3 + the block's downsample as ONE GEMM over [x ; x2], w and bias
// concatenated / summed by the caller): K grows by Cin2.  (The seam kernels' DS form sets x2 / Cin2 by plain assignment and
// leaves Ktot = Cin: conv_c3c1.hip never reads it.)
inline void conv_args_second_source(ConvArgs& a, const uint16_t* x2, const uint16_t* x2_lo, int Cin2) {
    a.x2 = x2;
    a.x2_lo = x2_lo;
    a.Cin2 = Cin2;
    a.Ktot = a.Cin + Cin2;
    a.T = a.Ktot / 64;
}
// The fused seam (conv_c3c1.hip): the following block's conv1 applied to this conv's output tile.
inline void conv_args_next_conv1(ConvArgs& a, const uint16_t* w2, const uint16_t* w2_lo, const float* bias2, uint16_t* y2,
                                 int Cout2, int relu2) {
    a.w2 = w2;
    a.w2_lo = w2_lo;
    a.bias2 = bias2;
    a.y2 = y2;
    a.Cout2 = Cout2;
    a.relu2 = relu2;
}

// ---- the variant table (conv_igemm.hip) ----------------------------------------------------------------------------------
typedef bool (*ConvAdmissibleFn)(const ConvArgs&);
typedef hipError_t (*ConvLaunchFn)(const ConvArgs&, int dtype, hipStream_t);

// One row per kernel configuration.  A row says when it applies and how it is launched; conv_variant_admissible and
// conv_launch only look the row up.  Rows keep their order and names: the index is what the tuner stores and exports.
struct ConvVariant {
    const char* name;
    int BM, BN, threads, stages, BK;   // tile, workgroup size, ring depth, K-step
    ConvAdmissibleFn admissible;       // the plain form, or nullptr (a two-source-only row)
    ConvLaunchFn launch;
    bool has_splitk;                   // launch honours ConvArgs::ksplit > 1 (conv_splitk_finalize then reduces the slices)
    ConvAdmissibleFn admissible_dual;  // the two-source form (ConvArgs::x2: conv3 + downsample in one GEMM), or nullptr
    ConvLaunchFn launch_dual;
};

// the kernels of the other sources that the table's rows bind
bool conv1x1_persist_admissible(const ConvArgs& a);                                 // conv_persist.hip: persistent 256 x 256 1x1
hipError_t conv1x1_persist_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv1x1_persist_x3_admissible(const ConvArgs& a);                              // ... with the pixel operand three K-steps deep (no residual)
hipError_t conv1x1_persist_x3_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv1x1_persist_dual_admissible(const ConvArgs& a);                            // ... and its two-source form
hipError_t conv1x1_persist_dual_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv_patch64_lc_admissible(const ConvArgs& a);                                 // conv_patchlc.hip
hipError_t conv_patch64_lc_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv1x1_ring_admissible(const ConvArgs& a);                                    // conv_ring.hip (experiments builds)
hipError_t conv1x1_ring_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv1x1_wreg_admissible(const ConvArgs& a);                                    // conv_wreg.hip
hipError_t conv1x1_wreg_launch(const ConvArgs& a, int dtype, hipStream_t stream);
// conv_small.hip - small maps: 64 x 64 tiles, four consumer + four loader waves, no workgroup barrier; an eight- or four-slot ring,
// or four slots of two K-steps each (K2: an even number of K-steps only)
bool conv_small_admissible(const ConvArgs& a);
bool conv_small_k2_admissible(const ConvArgs& a);
hipError_t conv_small_s8_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv_small_s4_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv_small_s4k2_launch(const ConvArgs& a, int dtype, hipStream_t stream);
// conv_persistlc.hip - the persistent 256 x 256 ring with loader / consumer roles: 1x1 without a residual (x2 unset) and its two-source form
bool conv1x1_lc_admissible(const ConvArgs& a);
bool conv1x1_lc_plain_admissible(const ConvArgs& a);
hipError_t conv1x1_lc_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv1x1_lc_dual_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv1x1_wregd_admissible(const ConvArgs& a);   // conv_wregd.hip: two-source form, K = 128 + 256 (layer2's first block)
hipError_t conv1x1_wregd_launch(const ConvArgs& a, int dtype, hipStream_t stream);
// the layer3 seam (planes 256): weights streamed from L2 through an LDS ring by loader waves (conv_seam3.hip); reached
// through conv_c3c1_admissible / conv_c3c1_launch like the register-stationary forms
bool conv_seam3_admissible(const ConvArgs& a);
hipError_t conv_seam3_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv_c3c1_admissible(const ConvArgs& a);
bool conv_c3c1ds_lc_admissible(const ConvArgs& a);   // the DS seam, loader / consumer form (conv_c3c1lc.hip)
hipError_t conv_c3c1ds_lc_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv_c3c1_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv_patch3x3s_admissible(const ConvArgs& a);
hipError_t conv_patch3x3s_launch(const ConvArgs& a, int dtype, hipStream_t stream);
bool conv_patch3x3w_admissible(const ConvArgs& a);
hipError_t conv_patch3x3w_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv_patch3x3w_pack(const uint16_t* w, uint16_t* out, int Cout, int Cin, hipStream_t stream);   // same size as w
bool conv_patch3x3s2_admissible(const ConvArgs& a);   // conv_patchs2.hip: 3x3 stride 2
hipError_t conv_patch3x3s2_launch(const ConvArgs& a, int dtype, hipStream_t stream);
hipError_t conv_patch3x3s2_pack(const uint16_t* w, uint16_t* out, int Cout, int Cin, hipStream_t stream);   // same size as w
bool conv_patch3x3_admissible(const ConvArgs& a);     // conv_patch.hip: Cin == Cout == 64 or 128
hipError_t conv_patch3x3_launch(const ConvArgs& a, int dtype, hipStream_t stream);

// Paired-fp16 convolution (conv_pair.hip): three fp16 MFMAs per product term (wh.xh + wh.xl + wl.xh) into one fp32
// accumulator; any R x S <= 4 x 4, stride, padding; Cin % 32 == 0, Cout % 64 == 0.  Returns a dir_status.
int conv_pair_launch(const ConvArgs& a, hipStream_t stream);
const char* conv_pair_variant_name(const ConvArgs& a);

int conv_variant_count();
const ConvVariant& conv_variant(int i);
bool conv_variant_admissible(int v, const ConvArgs& a);
int conv_pick_variant(const ConvArgs& a);
// Variant for the two-source form (a.x2 set), or -1 when none fits the shape.
int conv_pick_dual_variant(const ConvArgs& a, bool any_size = false);
int conv_launch(const ConvArgs& a, int dtype, int variant, hipStream_t stream);
// Split factor for variant `v` on problem `a` (1 = none) and the fp32 scratch it needs.
int conv_splitk_factor(int v, const ConvArgs& a);
size_t conv_splitk_bytes(const ConvArgs& a, int ksplit);
constexpr size_t kSplitKMaxBytes = 64u << 20;   // scratch the engine reserves for the partial sums
int conv_launch_naive(const ConvArgs& a, int dtype, hipStream_t stream);


}  // namespace dir

// conv_pick.hip — which tile kernel a convolution runs on when its shape has not been autotuned (host code only).
//
// conv_pick_variant is a chain of named rules in a fixed order - the order is behaviour: the first rule that returns a variant
// wins.  A rule reads the shape (ConvArgs), the tile counts derived from it once per call (PickShape), one snapshot of the A/B
// switches (Env) and the table rows it names (VariantIds: resolved from the names once per process).  The table itself
// (conv_igemm.hip) is reached only through conv_variant_count / conv_variant / conv_variant_admissible.
// A new rule is a new function and one line of the chain; a new row it names is one field and one line of VariantIds.
#include "dir_common.h"
#include "conv_igemm.h"

#include <string.h>
#include <algorithm>

namespace dir {

// ---- the rows the pickers name --------------------------------------------------------------------------------------------
// Field = the row's name (t<pixels>x<channels>... for the implicit-GEMM tiles).
struct VariantIds {
    int patchlc, patchs2, patch3x3_64, patch3x3_128, wreg, patchw, patchs, persist, persist_x3, lc1x1, wregd, small_s4k2;
    int t256x64_w4x1, t128x64_w2x2, t64x64_w2x1, t256x256_w4x4, t256x256_w4x2, t128x128_w2x2, t64x128_w2x2_s4, t64x128_w2x2;
    int t128x256_w2x4_s3_k32, t256x128_w4x2_s3, t256x128_w4x2_s3_k32, t64x64_w2x2_s4;
#ifdef DIR_EXPERIMENTS
    int ring;   // -1 where the build has no such row: its rule is skipped
#endif
    bool ok;    // every row a build must have was found; false = the pickers return -1 for every shape (a mistyped name below)
};

static int find_variant(const char* name) {
    for (int v = 0; v < conv_variant_count(); ++v)
        if (strcmp(conv_variant(v).name, name) == 0) return v;
    return -1;
}

static const VariantIds& variant_ids() {
    static const VariantIds ids = [] {
        static const struct { int VariantIds::*id; const char* name; } required[] = {
            {&VariantIds::patchlc, "256x64_patchlc3x3"},
            {&VariantIds::patchs2, "256x128_patchs2"},
            {&VariantIds::patch3x3_64, "256x64_patch3x3"},
            {&VariantIds::patch3x3_128, "256x128_patch3x3"},
            {&VariantIds::wreg, "64x512_wreg1x1"},
            {&VariantIds::patchw, "512x128_patch3x3w"},
            {&VariantIds::patchs, "256x256_patch3x3s"},
            {&VariantIds::persist, "256x256_persist1x1"},
            {&VariantIds::persist_x3, "256x256_persist1x1_x3"},
            {&VariantIds::lc1x1, "256x256_lc1x1"},
            {&VariantIds::wregd, "64x256_wregd1x1"},
            {&VariantIds::small_s4k2, "64x64_small_s4k2"},
            {&VariantIds::t256x64_w4x1, "256x64_w4x1"},
            {&VariantIds::t128x64_w2x2, "128x64_w2x2"},
            {&VariantIds::t64x64_w2x1, "64x64_w2x1"},
            {&VariantIds::t256x256_w4x4, "256x256_w4x4"},
            {&VariantIds::t256x256_w4x2, "256x256_w4x2"},
            {&VariantIds::t128x128_w2x2, "128x128_w2x2"},
            {&VariantIds::t64x128_w2x2_s4, "64x128_w2x2_s4"},
            {&VariantIds::t64x128_w2x2, "64x128_w2x2"},
            {&VariantIds::t128x256_w2x4_s3_k32, "128x256_w2x4_s3_k32"},
            {&VariantIds::t256x128_w4x2_s3, "256x128_w4x2_s3"},
            {&VariantIds::t256x128_w4x2_s3_k32, "256x128_w4x2_s3_k32"},
            {&VariantIds::t64x64_w2x2_s4, "64x64_w2x2_s4"},
        };
        VariantIds r;
        r.ok = true;
        for (const auto& q : required) {
            r.*q.id = find_variant(q.name);
            r.ok = r.ok && r.*q.id >= 0;
        }
#ifdef DIR_EXPERIMENTS
        r.ring = find_variant("128x256_ring1x1");
#endif
        return r;
    }();
    return ids;
}

// ---- what the rules ask of a shape, computed once per call ----------------------------------------------------------------
struct PickShape {
    int T;                // K-steps of 64
    bool spatial;         // the filter is larger than 1x1
    // tiles over the flattened pixels, <pixels>x<channels>: ceil(M / pixels) * (Cout / channels)
    long t256, t128, t64x128, t64, t64x512;
    long pw_flat_wgs;     // conv_patchw.hip counted the same way (512 pixels x 128 channels): what the small-map rules compare
    // per-image tiles of the patch kernels (a ragged map has more of them than its flattened pixels fill)
    long lc_tiles;        // 8 x 32 pixels (conv_patchlc.hip)
    long s2_tiles;        // 8 x 32 pixels x 128 channels (conv_patchs2.hip)
    long pw_image_wgs;    // 16 x 32 pixels x 128 channels: the workgroups conv_patchw.hip launches
    double pw_fill;       // ... and the part of their pixels that the map fills
};

static PickShape pick_shape(const ConvArgs& a) {
    PickShape s;
    s.T = a.Ktot / 64;
    s.spatial = a.R * a.S > 1;
    s.t256 = (long)ceil_div(a.M, 256) * (a.Cout / 256);
    s.t128 = (long)ceil_div(a.M, 128) * (a.Cout / 128);
    s.t64x128 = (long)ceil_div(a.M, 64) * (a.Cout / 128);
    s.t64 = (long)ceil_div(a.M, 64) * (a.Cout / 64);
    s.t64x512 = (long)ceil_div(a.M, 64) * (a.Cout / 512);
    s.pw_flat_wgs = (long)ceil_div(a.M, 512) * (a.Cout / 128);
    s.lc_tiles = (long)a.B * ((a.OH + 7) / 8) * ((a.OW + 31) / 32);
    s.s2_tiles = (long)a.B * ((a.OH + 7) / 8) * ((a.OW + 31) / 32) * (a.Cout / 128);
    const long pw_wgs = (long)a.B * ceil_div(a.OH, 16) * ceil_div(a.OW, 32) * (a.Cout / 128);
    s.pw_image_wgs = pw_wgs;
    s.pw_fill = a.Cout < 128 ? 0.0 : (double)a.M / ((double)(pw_wgs / (a.Cout / 128)) * 512.0);   // (read only where patchw is admissible)
    return s;
}

// ---- the rules, in the order conv_pick_variant tries them -----------------------------------------------------------------
// Each returns a variant or -1 (not mine: the next rule).

static int rule_patchlc(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    // layer1's 64 -> 64 3x3: filter resident in LDS, loader / consumer waves (DIRTORCH_AMD_NO_PATCHLC: A/B and bisecting)
    if (!e.no_patchlc && conv_variant_admissible(ids.patchlc, a) && s.lc_tiles >= 192) return ids.patchlc;
    return -1;
}

static int rule_patchs2(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    // 3x3 stride 2 over 128 channels (layer2.0's conv2, bound by its full-resolution input): the patch kernel with even / odd
    // column runs - 0.222 -> 0.208 ms standalone at batch 32 (gpurun_out/r6s2b).  Not for the 256 / 512-channel ones of
    // layer3.0 / 4.0: those are matrix-bound, and one plane in flight per CU costs them 15-25 us against the 16-wave tile (0.174
    // vs 0.149, 0.152 vs 0.135 ms) - the variant stays a tuner candidate there.  DIRTORCH_AMD_NO_PATCHS2: generic tiles again.
    if (!e.no_patchs2 && a.Cin <= 128 && conv_variant_admissible(ids.patchs2, a) && s.s2_tiles >= 192) return ids.patchs2;
    return -1;
}

static int rule_patch3x3(const ConvArgs& a, const PickShape&, const Env&, const VariantIds& ids) {
    // narrow 3x3 layers (Cin 64): conv_patch.hip's one-tile-of-Cout kernel, the row of the layer's channel count
    if (a.Cin != 64) return -1;
    if (conv_variant_admissible(ids.patch3x3_64, a)) return ids.patch3x3_64;
    if (conv_variant_admissible(ids.patch3x3_128, a)) return ids.patch3x3_128;
    return -1;
}

static int rule_wreg(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    // the residual 1x1 convs with K <= 256 (layer2/3 conv3): weights stationary in registers, as long
    // as every persistent workgroup gets at least ~4 pixel tiles to amortise loading them
    const bool no_wreg = e.no_wreg;   // A/B and bisecting
    if (!no_wreg && conv_variant_admissible(ids.wreg, a) && s.t64x512 >= 1024) return ids.wreg;
    return -1;
}

// The small-map regime (round 6, distilled from the tuner at batch 1 / batch 4 of 1024^2 and ResNet-50 at 64 x 224^2,
// gpurun_out/r6small): when a long-K layer with 256+ outputs cannot fill the chip with 256-wide tiles and 128 x 128 tiles give
// it less than two rounds, 64 x 128 tiles (48 KB: two workgroups per CU, one's fill under the other's MFMAs) are 8-10 %
// faster (same box: +0.5 % on the whole step at batch 4 and on config A); below ~250 of those, 64 x 64 tiles on a 4-slot ring
// (one per CU at 4 096 pixels x 256 channels, 64 KB so that a second stream's workgroup fits beside it).
static int rule_small_map(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    // (not where conv_patchw.hip, the list's first candidate, fills the chip - by its FLATTENED count)
    const bool patchw_fills = s.spatial && a.Cin >= 128 && !e.no_patchw && conv_patch3x3w_admissible(a) && s.pw_flat_wgs >= 192;
    if (e.no_smallmap || a.Cout % 256 != 0 || s.T < 6 || patchw_fills) return -1;
    if (s.t256 >= 192 || s.t128 >= 512) return -1;
    const int v1 = ids.t64x128_w2x2, v2 = ids.t64x64_w2x2_s4, v3 = ids.small_s4k2;
    const bool ok2 = conv_variant_admissible(v2, a), ok3 = conv_variant_admissible(v3, a);
    // Long K loops in this regime (the tuner at batch 4 of 1024^2 and ResNet-50 at 64 x 224^2, scripts/exp_tune_any.py):
    //   * layer4's 3x3 (K = 4608) with 96-191 tiles of 128 x 128: that tile with split-K (4 096 pixels x 512 channels: 62 -> 38 us
    //     per launch against the 64 x 128 tile, 3 136 pixels: 38 -> 33) - the small tiles stream the 4.7 MB filter once per 64 pixels;
    //   * layer4's 2048 -> 512 conv1 (32 K-steps): the 64 x 128 tile on its four-slot ring (33 -> 21 us), not the two-slot one.
    if (s.spatial && s.T >= 64 && s.t128 >= 96 && s.t128 < 192) {
        const int v4 = ids.t128x128_w2x2;
        if (conv_variant_admissible(v4, a)) return v4;
    }
    if (!s.spatial && s.t64x128 >= 256 && s.t64x128 < 384 && s.T >= 32) {   // (one workgroup per CU: no second one to hide the fill)
        const int v5 = ids.t64x128_w2x2_s4;
        if (conv_variant_admissible(v5, a)) return v5;
    }
    //   * 512+ output channels with 1.25+ rounds of 128 x 128 tiles (config A's layer4 1x1 convs, 392-400 tiles: 20-32 -> 17-24 us): the 64-pixel
    //     tile streams the wider weight matrix twice as often - those keep the list's 128 x 128 tile.
    const bool wide_n = a.Cout >= 512 && s.t128 >= 320;
    if (!wide_n && s.t64x128 >= 256 && conv_variant_admissible(v1, a)) return v1;
    if (s.t64x128 < 192 && s.t64 >= 192) {
        // (conv_small.hip's two-K-steps-per-stage tile is 8 % faster here on ONE stream - batch 1 at 1024^2 777 -> 839 img/s -
        // and, at 128 KB of LDS, 3-4 % slower on two to four: DIRTORCH_AMD_SMALL_K2 for callers that do not overlap forwards)
        if (e.small_k2 && ok3) return v3;
        if (ok2) return v2;
    }
    // Below 192 tiles of 64 x 64 the list further down fell to split-K on 64 x 128 tiles - a cliff native-size images sit right
    // under (683 x 1024: 43 x 64 pixels in layer3 = 172 tiles; the tuner, scripts/exp_batch1_tune.py: 16 -> 10 us per conv1).
    // conv_small.hip with two K-steps per stage instead, down to 32 tiles (layer4's 2048 -> 512 conv1 at 1024^2: 19 -> 14 us);
    // gpurun_out/r6b1rules, img/s on 1 / 2 / 4 streams: 683 x 1024 760 / 1128 / 1097 -> 960 / 1330 / 1287, 500 x 375 1010 /
    // 1590 / 1550 -> 1137 / 2100 / 2094, nothing lost at 1024^2 or 768 x 1024.  (K >= 4096, layer4's 3x3, keeps split-K.)
    if (s.t64x128 < 192 && s.t64 >= 32 && s.t64 < 192 && s.T < 64) {
        if (ok3) return v3;
        if (ok2) return v2;
    }
    return -1;
}

// Ragged maps (round 6, distilled from the tuner on configs[4]'s three scales, scripts/exp_multiscale_tune.py): the 16 x 32-pixel
// patch tile wastes what a map leaves of its last tiles (107^2: 20 %, 54^2: 29 %, 38^2: 53 %) where the implicit-GEMM tile walks
// the flattened pixels; both lose the idle part of their last round of workgroups.  With the 16-wave tile at 0.91 of the patch
// kernel's rate on full tiles (133 vs 121 us on layer3 at batch 32): 16 x 107^2 x 256 channels 0.70 vs 0.85 -> the flattened tile
// (tuner: 216 -> 201 us), 16 x 75^2 0.69 vs 0.63 and 16 x 54^2 0.71 vs 0.65 -> the patch kernel (tuner: the same), 16 x 38^2 x 512
// 0.35 vs 0.65 -> the flattened tile.  DIRTORCH_AMD_NO_SMALLMAP switches this off with the other distilled rules.
static int rule_ragged_map(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    if (!(s.spatial && a.Cin >= 128 && !e.no_patchw && conv_variant_admissible(ids.patchw, a))) return -1;
    const long pw_wgs = s.pw_image_wgs;
    const double fill = s.pw_fill;
    const int v_g = ids.t256x256_w4x4;
    if (!e.no_smallmap && a.Cout % 256 == 0 && conv_variant_admissible(v_g, a)) {
        auto round_eff = [](long wgs) { return (double)wgs / (double)(ceil_div((int)wgs, 256) * 256L); };
        const long t256 = s.t256;
        const double eff_p = fill * round_eff(pw_wgs);
        const double eff_g = 0.91 * round_eff(t256);
        if (t256 >= 176 && eff_g > 1.05 * eff_p) return v_g;
    }
    return -1;
}

// The candidates of a shape, largest tile first, each with the workgroups of it that share a CU.
struct Cand { int v; int wg_per_cu; };

static int candidate_list(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids, Cand c[12]) {
    const int T = s.T;
    int n = 0;
    {
        // 3x3 stride 1 over >= 128 channels (conv2 of layer2 / 3 / 4): 512 pixels x 128 channels per workgroup with
        // double-buffered 32-channel planes (conv_patchw.hip) - A/B at batch 32 (gpurun_out/pw): layer2 175 -> 153 us,
        // layer3 133 -> 124 us, layer4 121 -> 113 us.  Falls through (like every candidate) when it is not admissible
        // or leaves CUs without a tile.
        const bool no_pw = e.no_patchw;   // A/B and bisecting
        if (!no_pw && s.spatial && a.Cin >= 128) c[n++] = {ids.patchw, 1};
    }
    if (T <= 1 || a.Cout % 128 != 0) {
        c[n++] = {ids.t256x64_w4x1, 1}, c[n++] = {ids.t128x64_w2x2, 1}, c[n++] = {ids.t64x64_w2x1, 1};
    } else if (a.Cout % 256 == 0 && T >= 6) {
        // 3x3: 16 waves of 64x64; 1x1: the persistent kernel (falls through when not admissible)
        // 1x1 without a residual and a very long K loop (the 2048 -> 512 conv1 of layer4): the deep-X ring.
        // A/B at batch 32 (gpurun_out/r2b): 81 -> 71 us there, but 87 -> 90 us on layer3's 1024 -> 256 -
        // those are not short of HBM requests in flight, so they keep the 2-slot form.
        const bool no_x3 = e.no_x3;      // A/B and bisecting
        // Round 6: the tuner's pick flipped on layer3's 1024 -> 256 conv1 (22 launches; in-place identity blocks and the loader /
        // consumer 3x3 have changed what runs around it since round 2): 88-90 -> 82-84 us per launch, +0.9 % on the step
        // (gpurun_out/r6tune32).  256-channel outputs take the deep-X ring from K = 1024; DIRTORCH_AMD_X3_K2048 = the old rule.
        const bool x3 = !s.spatial && !a.res && !no_x3 && (T >= 32 || (T >= 16 && a.Cout <= 256 && !e.x3_k2048));
        // 3x3 over 256 / 512 channels: the plane-at-a-time patch kernel (conv_patch.hip) - falls through to the
        // 16-wave implicit-GEMM tile where it is not admissible (stride 2, odd widths) or too few tiles
        const bool no_ps = e.no_patchs;  // A/B and bisecting
        if (s.spatial && !no_ps) c[n++] = {ids.patchs, 1};
        // (conv_ring.hip's 128x256_ring1x1 - split loader / consumer waves - ties the persistent kernel on these layers
        // inside the network, gpurun_out/r3f-r3h: it stays a tuner candidate; an experiments build + DIRTORCH_AMD_EXPERIMENTS=1 puts it first, for A/B)
#ifdef DIR_EXPERIMENTS
        if (!s.spatial && !a.res && e.experiments) c[n++] = {ids.ring, 1};
#endif
        if (!s.spatial && !a.res && e.lc1x1) c[n++] = {ids.lc1x1, 1};   // (A/B: DIRTORCH_AMD_LC1X1)
        c[n++] = {s.spatial ? ids.t256x256_w4x4 : (x3 ? ids.persist_x3 : ids.persist), 1};
        c[n++] = {ids.t256x256_w4x2, 1}, c[n++] = {ids.t128x128_w2x2, 1};
        // small M (batch 1 at the deep stages): the 4-slot ring hides the fill latency of a long K
        // loop; with fewer than ~100 tiles even that leaves CUs idle and split-K takes over
        c[n++] = {ids.t64x128_w2x2_s4, 1}, c[n++] = {ids.t64x128_w2x2, 1};
    } else if (a.Cout % 256 == 0 && T >= 3) {
        c[n++] = {ids.t128x256_w2x4_s3_k32, 2}, c[n++] = {ids.t256x256_w4x2, 1}, c[n++] = {ids.t128x128_w2x2, 1};
        c[n++] = {ids.t128x64_w2x2, 1}, c[n++] = {ids.t64x64_w2x1, 1};   // short K: more, smaller tiles
    } else {
        // strided 3x3 (the first conv2 of layer2): the gather touches every other pixel, so the 128-B K rows of
        // the BK = 64 tile halve the number of requests per byte (A/B gpurun_out/r2t: 273 -> 224 us)
        if (s.spatial && a.stride > 1) c[n++] = {ids.t256x128_w4x2_s3, 1};
        c[n++] = {ids.t256x128_w4x2_s3_k32, 2}, c[n++] = {ids.t128x128_w2x2, 1};
        c[n++] = {T >= 8 ? ids.t64x128_w2x2_s4 : ids.t64x128_w2x2, 1}, c[n++] = {ids.t64x64_w2x1, 1};
    }
    return n;
}

// The first admissible candidate that gives about three quarters of the CU slots a tile; else the smallest tile.
static int rule_candidates(const ConvArgs& a, const PickShape& s, const Env& e, const VariantIds& ids) {
    Cand c[12];
    const int n = candidate_list(a, s, e, ids, c);
    // (set when the map fills at least 60 % of its tiles: a 7 x 7 map's one tile per image is no workgroup to count.  Read for
    // the patchw row alone, which is in the list only where rule_ragged_map counted it: 3x3, Cin >= 128, admissible)
    long pw_wgs = s.pw_image_wgs;
    if (s.pw_fill < 0.6) pw_wgs = 0;
    int last = -1, prev = -1;
    for (int i = 0; i < n; ++i) {
        const int v = c[i].v;
        if (!conv_variant_admissible(v, a)) continue;
        prev = last;
        last = v;
        // (the patch kernel's workgroups are per-image tiles: on a ragged map more than ceil(M / 512))
        const long tiles = v == ids.patchw && pw_wgs && !e.no_smallmap ? pw_wgs : (long)ceil_div(a.M, conv_variant(v).BM) * (a.Cout / conv_variant(v).BN);
        if (tiles >= 192L * c[i].wg_per_cu) return v;
    }
    // nothing fills the chip: the smallest tile, unless it is the split-K fallback of a list whose
    // deep-ring sibling still gets ~100 workgroups
    if (prev >= 0 && last >= 0 && conv_variant(last).has_splitk && prev == ids.t64x128_w2x2_s4 && s.t64x128 >= 96) return prev;
    return last;
}

// Heuristic used when a shape has not been autotuned (variable-size images, the reference's real
// workload).  Distilled from the autotuner's choices on ResNet-101 at 1024^2 (profiles/
// r01_tuned_variants_b32_1024.txt):
//   * narrow 3x3 layers (Cin 64) take the LDS-patch kernel, K = 64 layers the long 256x64 tile;
//   * wide outputs with a real K loop (layer3/4 conv1 + conv2) a 256x256 tile: the persistent
//     kernel for 1x1, the 16-wave form for 3x3;
//   * wide outputs with a short K loop (the 256 -> 1024 conv3 of layer3, residual + store bound)
//     and everything with 128/512 outputs (layer2) the 72 KB / 128-VGPR tiles that fit two
//     workgroups per CU, so that one's epilogue overlaps the other's K loop;
// each falling back to smaller pixel tiles until about three quarters of the CU slots get a tile.
int conv_pick_variant(const ConvArgs& a) {
    const VariantIds& ids = variant_ids();
    if (!ids.ok) return -1;
    const Env& e = env();
    const PickShape s = pick_shape(a);
    static int (*const rules[])(const ConvArgs&, const PickShape&, const Env&, const VariantIds&) = {
        rule_patchlc, rule_patchs2, rule_patch3x3, rule_wreg, rule_small_map, rule_ragged_map, rule_candidates};
    for (auto rule : rules)
        if (const int v = rule(a, s, e, ids); v >= 0) return v;
    return -1;
}

// Two-source form (conv3 + downsample of the first block of layers 2-4): the one kernel that carries it.
// History: conv_igemm.hip's own 256x256 tile (rounds 2-3: 0.359 / 0.261 / 0.206 ms on the first blocks of layers 2 / 3 / 4 where the
// persistent ring takes 0.311 / 0.238 / 0.197, bit-identical), a 3-slot 128x256 tile (0.39 / 0.29 / 0.22) and a split loader /
// consumer ring (0.357 / 0.267 / 0.224) were measured and retired.
int conv_pick_dual_variant(const ConvArgs& a, bool any_size) {
    const VariantIds& ids = variant_ids();
    const Env& e = env();
    const bool ok = a.x2 && a.R == 1 && a.S == 1 && a.stride == 1 && a.pad == 0 && a.H == a.OH && a.W == a.OW &&
                    a.Cin % 64 == 0 && a.Cin2 % 64 == 0 && a.res == nullptr && a.ksplit <= 1;
    if (!ok || !ids.ok) return -1;
    // (any_size: the op-level entry point runs the form on small shapes too - the tests')
    // layer2's first block (K = 128 + 256): weights stationary in registers, from ~4 pixel tiles per persistent workgroup
    // (round 6, A/B at batch 32 in profiles/r06_wregd.txt; DIRTORCH_AMD_NO_WREGD: the DUAL ring again)
    if (!e.no_wregd && conv1x1_wregd_admissible(a) &&
        (any_size || (long)ceil_div(a.M, 64) * (a.Cout / 256) >= 1024))
        return ids.wregd;
    if (a.Cout % 256 != 0 || (!any_size && (long)ceil_div(a.M, 256) * (a.Cout / 256) < 192)) return -1;
    // (conv_persistlc.hip - the same ring with loader / consumer wave roles - measured on layers 3-4, gpurun_out/r6lc1x1*: 4-8 % off the
    // launch by per-layer events, nothing on the whole step in two same-box A/Bs, and 5-15 % SLOWER on the plain 1x1 convs inside the
    // network; an opt-in (DIRTORCH_AMD_LC1X1) and a tuner candidate, not a default)
    if (e.lc1x1 && conv1x1_lc_admissible(a)) return ids.lc1x1;
    if (conv_variant(ids.persist_x3).launch_dual == nullptr) return -1;
    return ids.persist_x3;
}

// ---- split-K ---------------------------------------------------------------------------------------------------------------
size_t conv_splitk_bytes(const ConvArgs& a, int ksplit) {
    return ksplit > 1 ? (size_t)ksplit * a.M * a.Cout * sizeof(float) : 0;
}

// When a layer has too few output tiles to give every CU work (batch 1 at the deep stages), the K loop
// is cut into slices that run as separate workgroups.  Only the implicit-GEMM variants split, only
// when each slice keeps >= 4 K-steps, and only within the scratch the engine reserves.
int conv_splitk_factor(int v, const ConvArgs& a) {
    if (v < 0 || v >= conv_variant_count() || !conv_variant(v).has_splitk || a.Cin == 16) return 1;
    const ConvVariant& cv = conv_variant(v);
    const long tiles = (long)ceil_div(a.M, cv.BM) * (a.Cout / cv.BN);
    const int T = a.Ktot / cv.BK;
    if (tiles > 160 || T < 8) return 1;
    int s = (int)std::min<long>(std::min<long>(8, 512 / tiles), T / 4);
    while (s > 1 && conv_splitk_bytes(a, s) > kSplitKMaxBytes) --s;
    return s < 2 ? 1 : s;
}

}  // namespace dir

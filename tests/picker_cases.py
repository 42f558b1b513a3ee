"""The (tile variant, split-K factor) pairs the conv picker launches, one real layer shape each (a helper module like synth.py).

conv_pick_variant (csrc/conv_pick.hip) chooses a tile kernel per layer shape and conv_splitk_factor how many K slices it runs
in; the engine launches exactly that pair for every plain convolution it has not tuned.  PICKER_CASES holds one row per pair
the picker emits on the workloads this project claims (workload_layers), plus the launch forms those shapes do not reach:
persistent kernels walking several rounds of tiles with a ragged last one, split-K with K-steps that do not divide evenly, and
pairs only other channel counts reach.  tests/test_capi_host.py checks on the CPU that every row is still what the picker
returns and that nothing it returns lacks a row; tests/test_picker_parity_gpu.py runs every row against an fp32 reference.

Row: (tag, B, H, W, Cin, Cout, k, stride, pad, residual, relu, variant_name, ksplit) - NHWC input [B, H, W, Cin], a k x k
filter, the residual added before the ReLU.  Maps: the stem (stride 2) and the max-pool (stride 2) each take ceil(x / 2).
"""

CU_COUNT = 256           # MI355X: the persistent kernels' grid is min(work units, CUs)

# (name, arch, batch, image height, image width)
WORKLOADS = ([('r101_1024_b%d' % b, 'resnet101', b, 1024, 1024) for b in range(1, 33)] +           # the headline, batch 1-32
             [('native_%dx%d' % hw, 'resnet101', 1) + hw for hw in ((683, 1024), (1024, 683), (500, 375), (1023, 767), (768, 1024))] +
             [('ms%d_b%d' % (s, b), 'resnet101', b, s, s) for s in (848, 1200, 1697) for b in (1, 16)] +   # configs[4]: 1200^2 x 0.7071 / 1 / 1.4142
             [('r50_224_b%d' % b, 'resnet50', b, 224, 224) for b in (64, 128)])                          # config A

BLOCKS = {'resnet50': (3, 4, 6, 3), 'resnet101': (3, 4, 23, 3), 'resnet152': (3, 8, 36, 3)}


def _half(n):
    return (n - 1) // 2 + 1


def bottleneck_layers(arch, B, H, W):
    """Distinct conv shapes of a bottleneck ResNet's stack after the stem and the max-pool:
    [(layer, B, H, W, Cin, Cout, k, stride, pad, residual, relu)] - the stride on conv2, the 1x1 downsample of each first block
    (stride 1 in layer1), conv3 with its residual; blocks after the first share one shape per conv."""
    h, w, inplanes, out = _half(_half(H)), _half(_half(W)), 64, []
    for s, p in enumerate((64, 128, 256, 512)):
        st = 1 if s == 0 else 2
        oh, ow = (_half(h), _half(w)) if st == 2 else (h, w)
        out += [('layer%d.0.conv1' % (s + 1), B, h, w, inplanes, p, 1, 1, 0, False, True),
                ('layer%d.0.conv2' % (s + 1), B, h, w, p, p, 3, st, 1, False, True),
                ('layer%d.0.conv3' % (s + 1), B, oh, ow, p, 4 * p, 1, 1, 0, True, True),
                ('layer%d.0.downsample' % (s + 1), B, h, w, inplanes, 4 * p, 1, st, 0, False, False)]
        if BLOCKS[arch][s] > 1:
            out += [('layer%d.x.conv1' % (s + 1), B, oh, ow, 4 * p, p, 1, 1, 0, False, True),
                    ('layer%d.x.conv2' % (s + 1), B, oh, ow, p, p, 3, 1, 1, False, True),
                    ('layer%d.x.conv3' % (s + 1), B, oh, ow, p, 4 * p, 1, 1, 0, True, True)]
        h, w, inplanes = oh, ow, 4 * p
    return out


def workload_layers():
    """[(workload name, layer, B, H, W, Cin, Cout, k, stride, pad, residual, relu)] over WORKLOADS."""
    return [(name,) + l for name, arch, B, H, W in WORKLOADS for l in bottleneck_layers(arch, B, H, W)]


def launchable(B, H, W, Cin, Cout, k, stride, pad):
    """conv_launch's size limit (every tensor under 2^30 elements): the picker answers for larger shapes, the launch refuses."""
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return B * H * W * Cin < 1 << 30 and B * OH * OW * Cout < 1 << 30 and Cout * k * k * Cin < 1 << 30


def synthetic_grid():
    """A dense grid of launchable conv shapes: batch 1-128, maps 5-255 (odd, even, square and not), every conv of the
    bottleneck and basic-block ResNets and of the FPN head; then a coarser sweep of channel counts no ResNet has.
    [(B, H, W, Cin, Cout, k, stride, pad, residual)]."""
    types = [(2048, 1024, 1, 1, 0, False), (1024, 1024, 3, 1, 1, False)]          # FPN head: conv1x5, conv3c4
    for s, p in enumerate((64, 128, 256, 512)):
        inplanes, st = (64, 1) if s == 0 else (2 * p, 2)
        types += [(inplanes, p, 1, 1, 0, False), (4 * p, p, 1, 1, 0, False), (p, p, 3, 1, 1, False), (p, p, 3, st, 1, False),
                  (p, 4 * p, 1, 1, 0, True), (inplanes, 4 * p, 1, st, 0, False)]                       # bottleneck
        bin_ = 64 if s == 0 else p // 2
        types += [(bin_, p, 3, st, 1, False), (p, p, 3, 1, 1, True), (bin_, p, 1, st, 0, False)]      # basic block
    types = sorted(set(types))
    out = []
    for B in (1, 2, 3, 4, 5, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128):
        for h in (5, 7, 9, 11, 13, 14, 16, 19, 21, 25, 27, 28, 32, 33, 37, 38, 43, 47, 53, 54, 56, 64, 67, 75, 86, 96, 107,
                  112, 128, 150, 171, 192, 213, 224, 255):
            for w in sorted({h, max(5, h * 3 // 4), min(256, h * 4 // 3 + 1)}):
                out += [(B, h, w) + t for t in types if launchable(B, h, w, *t[:5])]
    chans = (64, 192, 384, 768, 1536, 4096)
    for B in (1, 2, 8, 32):
        for h in (7, 19, 38, 75, 150):
            for ci in chans:
                for co in chans:
                    for k, st, pad in ((1, 1, 0), (3, 1, 1), (3, 2, 1)):
                        for res in (False, True):
                            if launchable(B, h, h, ci, co, k, st, pad):
                                out.append((B, h, h, ci, co, k, st, pad, res))
    return out


PICKER_CASES = [
    # ---- one row per (variant, ksplit) the picker emits on WORKLOADS: the cheapest layer that lands on it, unless a row further
    # down already is one ------------------------------------------------------------------------------------------------------
    # (tag, B, H, W, Cin, Cout, k, stride, pad, residual, relu, variant, ksplit)
    ('native_683x1024.layer2.0.conv3', 1, 86, 128, 128, 512, 1, 1, 0, True, True, '128x128_w2x2', 1),        # T = 2 list: 256 x 128 short of 2 x 192, 344 tiles
    ('r101_1024_b5.layer4.x.conv2', 5, 32, 32, 512, 512, 3, 1, 1, False, True, '128x128_w2x2', 3),          # long-K small-map rule, 160 tiles -> split 3
    ('r101_1024_b4.layer4.x.conv2', 4, 32, 32, 512, 512, 3, 1, 1, False, True, '128x128_w2x2', 4),          # long-K small-map rule, 128 tiles -> split 4
    ('r101_1024_b3.layer3.0.conv3', 3, 64, 64, 256, 1024, 1, 1, 0, True, True, '128x256_w2x4_s3_k32', 1),   # short K (T = 4), 384 tiles
    ('native_683x1024.layer1.0.conv1', 1, 171, 256, 64, 64, 1, 1, 0, False, True, '128x64_w2x2', 1),        # T = 1 list, 256x64 short of 192
    ('r101_1024_b2.layer2.0.conv3', 2, 128, 128, 128, 512, 1, 1, 0, True, True, '256x128_w4x2_s3_k32', 1),  # 512 wreg tiles (< 1024), T = 2 list
    ('r101_1024_b12.layer3.x.conv1', 12, 64, 64, 1024, 256, 1, 1, 0, False, True, '256x256_persist1x1_x3', 1),   # 1x1, no residual, T >= 16
    ('r101_1024_b12.layer3.0.conv2', 12, 128, 128, 256, 256, 3, 2, 1, False, True, '256x256_w4x4', 1),     # strided 3x3 of 256 channels, 192 tiles
    ('native_500x375.layer1.0.conv2', 1, 125, 94, 64, 64, 3, 1, 1, False, True, '256x64_patch3x3', 1),      # 64 -> 64 3x3 under 192 lc tiles
    ('native_1023x767.layer1.0.conv1', 1, 256, 192, 64, 64, 1, 1, 0, False, True, '256x64_w4x1', 1),        # T = 1 list, 192 tiles of 256 x 64
    ('r101_1024_b6.layer2.x.conv2', 6, 128, 128, 128, 128, 3, 1, 1, False, True, '512x128_patch3x3w', 1),   # 3x3 over 128 channels, 192 tiles
    ('r101_1024_b1.layer4.0.conv3', 1, 32, 32, 512, 2048, 1, 1, 0, True, True, '64x128_w2x2', 1),           # small-map rule: 256 64 x 128 tiles
    ('native_500x375.layer4.x.conv1', 1, 16, 12, 2048, 512, 1, 1, 0, False, True, '64x128_w2x2', 8),         # 12 tiles, < 32 of 64 x 64: split-K
    ('ms848_b1.layer4.0.conv3', 1, 27, 27, 512, 2048, 1, 1, 0, True, True, '64x128_w2x2_s4', 1),             # fallback: deep-ring sibling >= 96 tiles
    ('native_500x375.layer3.x.conv1', 1, 32, 24, 1024, 256, 1, 1, 0, False, True, '64x64_small_s4k2', 1),     # 48 tiles of 64 x 64 (32-191)
    ('native_500x375.layer1.0.conv1', 1, 125, 94, 64, 64, 1, 1, 0, False, True, '64x64_w2x1', 1),            # T = 1 list, nothing fills the chip
    ('native_500x375.layer3.0.downsample', 1, 63, 47, 512, 1024, 1, 2, 0, False, False, '64x64_w2x2_s4', 1),  # 192 tiles of 64 x 64, 96 of 64 x 128
    # ---- persistent kernels: work units > grid (min(units, 256 CUs)), >= 2 rounds, not a multiple of the grid, ragged last pixel
    # tile - workgroups walk several tiles, the channel tile changes between them, the last round is short
    ('ms1697_b1.layer1.0.conv2', 1, 425, 425, 64, 64, 3, 1, 1, False, True, '256x64_patchlc3x3', 1),        # 54 x 14 = 756 tiles of 8 x 32
    ('ms848_b16.layer2.0.conv2', 16, 212, 212, 128, 128, 3, 2, 1, False, True, '256x128_patchs2', 1),       # 106^2 outputs: 896 tiles
    ('ms848_b16.layer3.0.conv1', 16, 106, 106, 512, 256, 1, 1, 0, False, True, '256x256_persist1x1', 1),    # 703 tiles, 64 pixels in the last
    ('grid.b96_r101_layer3.x.conv1', 96, 37, 37, 1024, 256, 1, 1, 0, False, True, '256x256_persist1x1_x3', 1),   # 514 tiles (a 592^2 batch)
    ('ms848_b16.layer3.0.conv3', 16, 53, 53, 256, 1024, 1, 1, 0, True, True, '64x512_wreg1x1', 1),          # 703 pixel tiles x 2 slices on 256
    ('grid.b96_r101_layer2.x.conv2', 96, 33, 33, 128, 128, 3, 1, 1, False, True, '512x128_patch3x3w', 1),   # 576 workgroups (one tile each), 2 x 2 per image
    # ---- split-K whose K-steps the slices do not share evenly (T = K / 64): the last slice is short ------------------------------
    ('r50_224_b64.layer4.0.conv2', 64, 14, 14, 512, 512, 3, 2, 1, False, True, '128x128_w2x2', 5),          # config A; T = 72 = 5 x 14 + 2
    ('ms1200_b1.layer4.0.conv2', 1, 75, 75, 512, 512, 3, 2, 1, False, True, '64x128_w2x2', 5),              # configs[4] batch 1; T = 72
    ('grid.r34_layer3.x.conv2', 1, 5, 5, 256, 256, 3, 1, 1, True, True, '64x128_w2x2', 8),                  # + residual; T = 36 = 8 x 4 + 4
    ('grid.r18_layer3.0.conv1', 1, 5, 5, 128, 256, 3, 2, 1, False, True, '64x128_w2x2', 4),                 # T = 18 = 4 x 4 + 2
    ('grid.r101_layer4.0.conv2', 8, 19, 26, 512, 512, 3, 2, 1, False, True, '64x128_w2x2', 7),              # 70 tiles; T = 72 = 7 x 10 + 2
    # ---- split-K pairs only channel counts outside ResNet reach (the grid's second sweep); uneven where the grid has such a shape
    ('grid.c64_to_768_s2', 1, 7, 7, 64, 768, 3, 2, 1, True, False, '64x128_w2x2', 2),                      # + residual, no ReLU; T = 9
    ('grid.c768_1x1', 1, 7, 7, 768, 768, 1, 1, 0, False, True, '64x128_w2x2', 3),                          # T = 12 (no uneven shape picks /3)
    ('grid.c192_to_768_s2', 1, 7, 7, 192, 768, 3, 2, 1, False, True, '64x128_w2x2', 6),                    # T = 27 = 6 x 4 + 3
    ('grid.c64_to_4096_s2', 1, 7, 7, 64, 4096, 3, 2, 1, False, True, '64x64_w2x2_s4', 2),                  # T = 9
    ('grid.c192_to_1536', 1, 19, 19, 192, 1536, 3, 1, 1, True, True, '64x64_w2x2_s4', 3),                  # + residual; T = 27 = 3 x 9
    ('grid.c192_to_4096_s2', 1, 19, 19, 192, 4096, 3, 2, 1, False, True, '64x64_w2x2_s4', 4),              # T = 27 = 4 x 6 + 3
    ('grid.c192_to_1536_s2', 2, 19, 19, 192, 1536, 3, 2, 1, False, False, '64x64_w2x2_s4', 5),             # no ReLU; T = 27 = 5 x 5 + 2
    ('grid.c192_to_4096_s2_b1_7', 1, 7, 7, 192, 4096, 3, 2, 1, True, True, '64x64_w2x2_s4', 6),            # + residual; T = 27 = 6 x 4 + 3
    # ---- other pairs only channel counts outside ResNet reach.  256x256_patch3x3s has no row: the picker
    # returns it only where 512x128_patch3x3w is not admissible, i.e. over conv_launch's size limit ---------------------------------
    ('grid.c192_to_4096', 2, 38, 38, 192, 4096, 1, 1, 0, False, False, '256x256_w4x2', 1),                   # T = 3: 192 tiles of 256 x 256
    ('grid.c64_to_384_s2_res', 1, 256, 256, 64, 384, 3, 2, 1, True, True, '256x128_w4x2_s3', 1),             # strided 3x3 + residual, no patch kernel
]

PERSISTENT = ('patchlc3x3', 'patchs2', 'persist1x1', 'wreg1x1', 'patch3x3w')   # (name fragments; persist1x1 covers _x3)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def k_steps(Cin, k):
    """T: K-steps of 64 (the split-K variants' BK)."""
    return k * k * Cin // 64


def launch_geometry(variant, B, H, W, Cin, Cout, k, stride, pad):
    """(work units, workgroups, ragged last pixel tile) of a persistent-style launch, mirroring its launcher, or None.
    conv_patchlc / patchs2 / persist: units = tiles, grid min(tiles, CUs); conv_wreg: pixel tiles of 64 x the 512-channel
    slices on min(256 / slices, pixel tiles) workgroups per slice; conv_patchw: one 16 x 32 tile per workgroup, all launched."""
    OH, OW = out_hw(H, W, k, stride, pad)
    M = B * OH * OW
    cdiv = lambda a, b: -(-a // b)
    if 'patchlc3x3' in variant:
        t = B * cdiv(OH, 8) * cdiv(OW, 32)
        return t, min(t, CU_COUNT), bool(OH % 8 or OW % 32)
    if 'patchs2' in variant:
        t = B * cdiv(OH, 8) * cdiv(OW, 32) * (Cout // 128)
        return t, min(t, CU_COUNT), bool(OH % 8 or OW % 32)
    if 'persist1x1' in variant:
        t = cdiv(M, 256) * (Cout // 256)
        return t, min(t, CU_COUNT), bool(M % 256)
    if 'wreg1x1' in variant:
        nsl, mt = Cout // 512, cdiv(M, 64)
        return mt * nsl, min(CU_COUNT // nsl, mt) * nsl, bool(M % 64)
    if 'patch3x3w' in variant:
        t = B * cdiv(OH, 16) * cdiv(OW, 32) * (Cout // 128)
        return t, CU_COUNT, bool(OH % 16 or OW % 32)    # (one tile per workgroup: "rounds" of 256 CUs)
    return None


def walks_rounds(variant, row_shape):
    """The persistent row property: >= 2 rounds of the grid, not a multiple of it, a ragged last pixel tile."""
    g = launch_geometry(variant, *row_shape)
    return g is not None and g[0] >= 2 * g[1] and g[0] % g[1] != 0 and g[2]

"""The engine's fused, paired and stem launches, one row per launch form and walk regime (a helper module like picker_cases.py).

csrc/engine.hip's forward launches, besides the plain convolutions the picker chooses (picker_cases.py), the layer1-2 seams
(conv_c3c1.hip, conv_c3c1lc.hip: run_seam, from kSeamMinTiles = 2048 pixel tiles of 64), the two-source conv3 + downsample GEMMs
(conv_wregd.hip, conv_persist.hip DUAL: conv_pick_dual_variant, from 1024 / 192 work units), the paired convolutions of the fp16p
head (conv_pair.hip: run_conv_pair) and the stems (stem_pool.hip, stem_u8.hip).  They are persistent or walk a sequence of tiles on
min(tiles, CUs) workgroups - conv_pair, one workgroup per tile, is the exception - so a row is a launch FORM (the profile label the
engine records, plus the sub-form the label does not say) at a shape whose walk puts it in one REGIME:
  first    the smallest claimed workload at which the engine picks the form;
  largest  the largest one (the index products closest to 2^30 elements);
  walk     three or more tiles per workgroup, a tile count that is not a multiple of the grid, a ragged last tile (may be synthetic);
  one      fewer tiles than workgroup slots: each workgroup takes one tile or none.
engine_launches() mirrors the engine's choice of these launches per (workload, dtype, feed); tests/test_capi_host.py checks the table
against it and launch_geometry() on the CPU, and tests/test_engine_launch_parity_gpu.py checks the mirror against the engine's own
launch record and runs every row against a high-precision CPU reference.

Row: (tag, label, sub, workload, record, shape, dtypes).  workload is a WORKLOADS name - the row is then that workload's launch - or
'synthetic' (walk and one-tile rows only: a shape of today's small-shape tests, named in `record`); record the engine's profile name of
the launch (layerS.J.c3c1, layer1.0.ds+c3c1, layerS.0.ds+conv3, layer1.J.conv1 / conv3 / downsample, conv1+maxpool); shape the
operands (SHAPE_FIELDS of the family).
"""
from picker_cases import BLOCKS, CU_COUNT, WORKLOADS, bottleneck_layers

SEAM_MIN_TILES = 2048        # engine.hip kSeamMinTiles
WREGD_MIN_UNITS = 1024       # conv_pick_dual_variant: 64-pixel tiles x 256-channel slices
X3_MIN_UNITS = 192           # ... 256 x 256 tiles
STEM_SLOTS = 2 * CU_COUNT    # the walking stems run two 4-wave workgroups per CU

# operand fields per family: seam (conv_c3c1<..>) = t2 map and planes; dual = conv3's output map, the downsample source and its stride;
# pair = one convolution; stem = the image
SHAPE_FIELDS = {
    'seam': ('B', 'H', 'W', 'P', 'P2', 'relu3', 'relu1'),
    'dual': ('B', 'OH', 'OW', 'Cin', 'Cin2', 'H2', 'W2', 'stride2', 'Cout', 'relu'),
    'pair': ('B', 'H', 'W', 'Cin', 'Cout', 'k', 'stride', 'residual', 'relu'),
    'stem': ('B', 'H', 'W'),
}


def family(label):
    if label.startswith('conv_c3c1<'):
        return 'seam'
    if label.endswith('/dual>'):
        return 'dual'
    if label.startswith('conv_pair<'):
        return 'pair'
    assert label.startswith('stem_pool'), label
    return 'stem'


def _cdiv(a, b):
    return -(-a // b)


def _workload(name):
    for w in WORKLOADS:
        if w[0] == name:
            return w
    raise KeyError(name)


def _layer(arch, B, H, W, name):
    """bottleneck_layers' tuple for 'layerS.J.conv' (J > 0 is the shared 'layerS.x.conv' shape)."""
    s, j, conv = name.split('.')
    key = '%s.%s.%s' % (s, '0' if j == '0' else 'x', conv)
    for l in bottleneck_layers(arch, B, H, W):
        if l[0] == key:
            return l
    raise KeyError((arch, name))


def layer_shape(workload, record, label):
    """The operands of the launch `label` would make for `record` of a claimed workload (SHAPE_FIELDS order)."""
    _, arch, B, H, W = _workload(workload)
    fam = family(label)
    if fam == 'stem':
        assert record == 'conv1+maxpool', record
        return (B, H, W)
    s, j, what = record.split('.')
    S, J = int(s[5:]), int(j)
    if fam == 'seam':
        c3 = _layer(arch, B, H, W, 'layer%d.%d.conv3' % (S, J))
        nxt = ('layer%d.%d.conv1' % (S, J + 1)) if J + 1 < BLOCKS[arch][S - 1] else ('layer%d.0.conv1' % (S + 1))
        c1 = _layer(arch, B, H, W, nxt)
        assert c1[4] == c3[5] and c1[2:4] == c3[2:4]
        return (B, c3[2], c3[3], c3[4], c1[5], True, True)
    if fam == 'dual':
        c3 = _layer(arch, B, H, W, 'layer%d.0.conv3' % S)
        ds = _layer(arch, B, H, W, 'layer%d.0.downsample' % S)
        return (B, c3[2], c3[3], c3[4], ds[4], ds[2], ds[3], ds[7], c3[5], True)
    l = _layer(arch, B, H, W, record)
    return (B, l[2], l[3], l[4], l[5], l[6], l[7], l[9], l[10])


def stem_maps(H, W):
    """(OH, OW, PH, PW): the 7x7 s2 p3 conv, then the 3x3 s2 p1 max-pool."""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return OH, OW, (OH - 1) // 2 + 1, (OW - 1) // 2 + 1


def stem_walk_segments(B, PH, PW):
    """stem_pool_u8_launch / stem_pool_pair_walk_launch (stem_u8.hip): items = (segment, image, 15-pixel column strip), each a run
    of T conv tiles; T halves from 8 while fewer than two items per workgroup slot result.  -> (seg_rows, items)."""
    tiles_x, T = _cdiv(PW, 15), 8
    while T > 1 and B * tiles_x * _cdiv(PH, 4 * T - 1) < 2 * STEM_SLOTS:
        T >>= 1
    seg = 4 * T - 1
    return seg, B * tiles_x * _cdiv(PH, seg)


def launch_geometry(form, shape):
    """(work units, workgroups, ragged last pixel tile) of a launch, mirroring its launcher:
    launch_c3c1 / conv_c3c1ds_lc_launch (conv_c3c1.hip, conv_c3c1lc.hip): 64-pixel tiles on min(tiles, CUs);
    launch_wregd (conv_wregd.hip): 64-pixel tiles x Cout / 256 slices, per = min(CUs / slices, tiles) workgroups per slice;
    launch_persist (conv_persist.hip): 256 x 256 tiles on min(tiles, CUs);
    launch_pair (conv_pair.hip): 128-pixel x 128- (64-) channel tiles, one workgroup each;
    stem_pool_u8_launch / stem_pool_pair_walk_launch: (segment, image, strip) items on min(items, 2 CUs);
    stem_pool_launch (persistent form): 3 x 15 pooled tiles on min(tiles, 2 CUs)."""
    label, sub = form
    fam = family(label)
    if fam == 'seam':
        M = shape[0] * shape[1] * shape[2]
        t = _cdiv(M, 64)
        return t, min(t, CU_COUNT), bool(M % 64)
    if fam == 'dual':
        B, OH, OW, Cin, Cin2, H2, W2, s2, Cout = shape[:9]
        M = B * OH * OW
        if 'wregd' in label:
            nsl, mt = Cout // 256, _cdiv(M, 64)
            per = min(max(CU_COUNT // nsl, 1), mt)
            return mt * nsl, per * nsl, bool(M % 64)
        t = _cdiv(M, 256) * (Cout // 256)
        return t, min(t, CU_COUNT), bool(M % 256)
    if fam == 'pair':
        B, H, W, Cin, Cout, k, stride = shape[:7]
        OH, OW = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
        M = B * OH * OW
        t = _cdiv(M, 128) * (Cout // (128 if Cout % 128 == 0 else 64))
        return t, t, bool(M % 128)
    B, H, W = shape
    _, _, PH, PW = stem_maps(H, W)
    if label in ('stem_pool_u8', 'stem_pool_pair'):
        seg, items = stem_walk_segments(B, PH, PW)
        return items, min(items, STEM_SLOTS), bool(PW % 15 or PH % seg)
    t = B * _cdiv(PH, 3) * _cdiv(PW, 15)
    return t, min(t, STEM_SLOTS), bool(PH % 3 or PW % 15)


def walk_position(form, shape, m, n):
    """Where output element (pixel m, channel n) sits in its launch's walk, mirroring each kernel's work order:
    (work unit, logical workgroup, walk step, what a unit is).  Logical workgroups are before the XCD remap of conv_wregd /
    conv_persist.  m counts output pixels over [B, OH, OW] (the stems: pooled pixels over [B, PH, PW])."""
    label, sub = form
    fam = family(label)
    units, grid, _ = launch_geometry(form, shape)
    if fam == 'seam':       # conv_c3c1 / conv_c3c1lc: tile = blockIdx.x, += gridDim.x
        t = m // 64
        return t, t % grid, t // grid, '64-pixel tile'
    if fam == 'dual' and 'wregd' in label:     # workgroup g: channel slice g % nsl, pixel tiles g / nsl + i * per
        nsl = shape[8] // 256
        per = grid // nsl
        t = m // 64
        return t * nsl + n // 256, (t % per) * nsl + n // 256, t // per, '64-pixel tile x 256-channel slice'
    if fam == 'dual':       # conv_persist: tile = tile_m * tiles_n + tile_n, += gridDim.x
        u = (m // 256) * (shape[8] // 256) + n // 256
        return u, u % grid, u // grid, '256 x 256 tile'
    if fam == 'pair':       # one workgroup per tile
        BN = 128 if shape[4] % 128 == 0 else 64
        u = (m // 128) * (shape[4] // BN) + n // BN
        return u, u, 0, '128 x %d tile' % BN
    B, H, W = shape
    _, _, PH, PW = stem_maps(H, W)
    b, ph, pw = m // (PH * PW), (m // PW) % PH, m % PW
    if label in ('stem_pool_u8', 'stem_pool_pair'):     # item = (segment, image, 15-pixel strip), += gridDim.x
        seg, _ = stem_walk_segments(B, PH, PW)
        u = ((ph // seg) * B + b) * _cdiv(PW, 15) + pw // 15
        return u, u % grid, u // grid, '(segment, image, strip) item'
    u = (b * _cdiv(PH, 3) + ph // 3) * _cdiv(PW, 15) + pw // 15     # stem_pool: 3 x 15 pooled tiles, += gridDim.x
    return u, u % grid, u // grid, '3 x 15 pooled tile'


def regimes(form, shape):
    """The geometric regimes of a row: 'walk' and / or 'one' (first / largest depend on the workloads: form_extremes)."""
    units, grid, ragged = launch_geometry(form, shape)
    out = set()
    if units >= 3 * grid and units % grid != 0 and ragged:
        out.add('walk')
    if units <= grid:
        out.add('one')
    return out


def walks(form):
    """False for the kernels that launch one workgroup per tile (conv_pair): they have no walk regime."""
    return family(form[0]) != 'pair'


# ---- the mirror of the engine's choices (csrc/engine.hip forward / forward_pair_stem / run_seam / run_conv_dual) --------------------
def engine_launches(workload, dtype, feed):
    """[(record, label, sub)] of the in-scope launches one forward of `workload` makes, default switches, bottleneck nets.
    dtype in bf16 / fp16 / fp16p (paired 1x1 weights in layer1: DIRTORCH_AMD_PAIR_STAGES = 1), feed in u8 (NHWC) / f32 (NCHW)."""
    _, arch, B, H, W = _workload(workload)
    pair = dtype == 'fp16p'
    out = []
    if pair and feed == 'u8':
        out.append(('conv1+maxpool', 'stem_pool_u8', 'raw' if W % 2 == 0 and B * H * W * 3 < 1 << 31 else 'prep'))
    elif pair:
        out.append(('conv1+maxpool', 'stem_pool_pair', 'walk' if W % 2 == 0 and B * 3 * H * W * 4 < 1 << 31 else 'twokernel'))
    else:
        out.append(('conv1+maxpool', 'stem_pool', 'persist'))
    blocks = [(s, j) for s in range(1, 5) for j in range(BLOCKS[arch][s - 1])]
    t1_ready = False
    for bi, (s, j) in enumerate(blocks):
        c3 = _layer(arch, B, H, W, 'layer%d.%d.conv3' % (s, j))
        M = B * c3[2] * c3[3]
        P, C = c3[4], c3[5]
        paired = pair and s == 1                  # layer1's 1x1 weights are pairs (engine.hip finalize: is_pair)
        cur_lo = pair and bi == 0                 # the block input has a lo plane: the stem's pooled output
        seam_next = bi + 1 < len(blocks)
        tiles = _cdiv(M, 64)
        ds_in_seam = (j == 0 and s == 1 and seam_next and BLOCKS[arch][0] > 1 and tiles >= SEAM_MIN_TILES and M * C < 1 << 30)
        dual = None
        if j == 0 and not ds_in_seam and not cur_lo and not paired:
            ds = _layer(arch, B, H, W, 'layer%d.0.downsample' % s)
            if P == 128 and ds[4] == 256 and c3[3] > 1 and tiles * (C // 256) >= WREGD_MIN_UNITS:
                dual = '64x256_wregd1x1'
            elif C % 256 == 0 and _cdiv(M, 256) * (C // 256) >= X3_MIN_UNITS:
                dual = '256x256_persist1x1_x3'
        pre = 'layer%d.%d' % (s, j)
        if j == 0 and not ds_in_seam and not dual and paired:
            out.append((pre + '.downsample', 'conv_pair<128x128_%s>' % ('xw' if cur_lo else 'w'), None))
        if not t1_ready and paired:
            out.append((pre + '.conv1', 'conv_pair<128x64_%s>' % ('xw' if cur_lo else 'w'), None))
        t1_ready = False
        if dual:      # (the x3 ring's second source: layer1's stride-1 block input or a stride-2 one)
            out.append((pre + '.ds+conv3', 'conv_igemm<%s/dual>' % dual, None if 'wregd' in dual else 'ds_stride%d' % (1 if s == 1 else 2)))
            continue
        seam = None
        if seam_next:
            c1 = _layer(arch, B, H, W, ('layer%d.%d.conv1' % (s, j + 1)) if j + 1 < BLOCKS[arch][s - 1] else ('layer%d.0.conv1' % (s + 1)))
            P2, w1_pair = c1[5], pair and c1[0].startswith('layer1.')
            ok = P in (64, 128) and (P2 == P or (P == 64 and P2 == 128 and not ds_in_seam)) and M * C < 1 << 30 and tiles >= SEAM_MIN_TILES
            if paired:
                ok = ok and (w1_pair or P2 == 128)
            if ds_in_seam:
                seam = (pre + '.ds+c3c1', 'conv_c3c1<64,ds%s>' % (',wp' if paired else ''), 'lc')
            elif ok:
                sub = 'p2_%d' % P2 + ('' if not paired else ('_w1pair' if w1_pair else '_w1single'))
                seam = (pre + '.c3c1', 'conv_c3c1<%d%s>' % (P, ',wp' if paired else ''), sub if P == 64 else None)
        if seam:
            out.append(seam)
            t1_ready = True
        elif paired:
            out.append((pre + '.conv3', 'conv_pair<128x128_w>', None))
    return out


FEEDS = {'bf16': ('u8', 'f32'), 'fp16': ('u8', 'f32'), 'fp16p': ('u8', 'f32')}


def all_launches():
    """{(label, sub): [(workload, record, dtype, feed)]} over every claimed workload, dtype and feed."""
    out = {}
    for wl in WORKLOADS:
        for dt, feeds in FEEDS.items():
            for feed in feeds:
                for rec, label, sub in engine_launches(wl[0], dt, feed):
                    out.setdefault((label, sub), []).append((wl[0], rec, dt, feed))
    return out


def form_extremes(form, launches):
    """(smallest, largest) work units of a form over its claimed launches: the first / largest regime rows must sit there."""
    units = [launch_geometry(form, layer_shape(wl, rec, form[0]))[0] for wl, rec, _, _ in launches]
    return min(units), max(units)


SEAM = lambda B, H, W, P, P2: (B, H, W, P, P2, True, True)      # noqa: E731
STEM = lambda B, H, W: (B, H, W)                                  # noqa: E731
_L1, _L2 = ('bf16', 'fp16'), ('fp16p',)

# (tag, label, sub, workload, record, shape, dtypes); the comment gives (work units / workgroups) and the regimes
ENGINE_CASES = [
    # ---- conv_c3c1<64>, P2 = 64: layer1's seams (conv3 of block J + conv1 of block J + 1) --------------------------------------
    ('seam64.first', 'conv_c3c1<64>', 'p2_64', 'r101_1024_b2', 'layer1.1.c3c1', SEAM(2, 256, 256, 64, 64), _L1),      # 2048 / 256
    ('seam64.largest', 'conv_c3c1<64>', 'p2_64', 'ms1697_b16', 'layer1.1.c3c1', SEAM(16, 425, 425, 64, 64), _L1),   # 45157: 177 odd, walk
    ('seam64.one', 'conv_c3c1<64>', 'p2_64', 'synthetic', 'SEAM_SHAPES', SEAM(2, 37, 29, 64, 64), _L1),            # 34 tiles
    # ---- conv_c3c1<64>, P2 = 128: layer1's last seam, into layer2.0.conv1 ------------------------------------------------------------
    ('seam64to128.first', 'conv_c3c1<64>', 'p2_128', 'r101_1024_b2', 'layer1.2.c3c1', SEAM(2, 256, 256, 64, 128), _L1),
    ('seam64to128.largest', 'conv_c3c1<64>', 'p2_128', 'ms1697_b16', 'layer1.2.c3c1', SEAM(16, 425, 425, 64, 128), _L1),
    ('seam64to128.one', 'conv_c3c1<64>', 'p2_128', 'synthetic', 'SEAM_SHAPES', SEAM(1, 5, 7, 64, 128), _L1),
    # ---- conv_c3c1<64,ds>: layer1's first block, the downsample as extra K, role-split kernel (conv_c3c1lc.hip) -------------------
    ('ds_seam.first', 'conv_c3c1<64,ds>', 'lc', 'r101_1024_b2', 'layer1.0.ds+c3c1', SEAM(2, 256, 256, 64, 64), _L1),
    ('ds_seam.largest', 'conv_c3c1<64,ds>', 'lc', 'ms1697_b16', 'layer1.0.ds+c3c1', SEAM(16, 425, 425, 64, 64), _L1),   # odd pair loop
    ('ds_seam.walk_even', 'conv_c3c1<64,ds>', 'lc', 'ms1697_b1', 'layer1.0.ds+c3c1', SEAM(1, 425, 425, 64, 64), _L1),
    ('ds_seam.one', 'conv_c3c1<64,ds>', 'lc', 'synthetic', 'SEAM_SHAPES', SEAM(2, 37, 29, 64, 64), _L1),
    # ---- conv_c3c1<128>: layer2's seams -----------------------------------------------------------------------------------------
    ('seam128.first', 'conv_c3c1<128>', None, 'r101_1024_b8', 'layer2.1.c3c1', SEAM(8, 128, 128, 128, 128), _L1),   # 2048
    ('seam128.largest', 'conv_c3c1<128>', None, 'ms1697_b16', 'layer2.1.c3c1', SEAM(16, 213, 213, 128, 128), _L1 + _L2),   # 11343, walk
    ('seam128.one', 'conv_c3c1<128>', None, 'synthetic', 'SEAM_SHAPES', SEAM(2, 37, 29, 128, 128), _L1),
    # ---- conv_c3c1<64,wp>: fp16p's layer1 seams with paired weights (WP3; WP1 where conv1 is layer1's) ------------------------------
    ('wp_seam64.first', 'conv_c3c1<64,wp>', 'p2_64_w1pair', 'r101_1024_b2', 'layer1.1.c3c1', SEAM(2, 256, 256, 64, 64), _L2),
    ('wp_seam64.largest', 'conv_c3c1<64,wp>', 'p2_64_w1pair', 'ms1697_b16', 'layer1.1.c3c1', SEAM(16, 425, 425, 64, 64), _L2),
    ('wp_seam64.one', 'conv_c3c1<64,wp>', 'p2_64_w1pair', 'synthetic', 'test_seam_with_paired_weights', SEAM(1, 9, 13, 64, 64), _L2),
    ('wp_seam128.first', 'conv_c3c1<64,wp>', 'p2_128_w1single', 'r101_1024_b2', 'layer1.2.c3c1', SEAM(2, 256, 256, 64, 128), _L2),
    ('wp_seam128.largest', 'conv_c3c1<64,wp>', 'p2_128_w1single', 'ms1697_b16', 'layer1.2.c3c1', SEAM(16, 425, 425, 64, 128), _L2),
    ('wp_seam128.one', 'conv_c3c1<64,wp>', 'p2_128_w1single', 'synthetic', 'test_seam_with_paired_weights', SEAM(2, 16, 16, 64, 128), _L2),
    # ---- conv_c3c1<64,ds,wp>: ... and the downsample form, paired block input (the stem's lo plane) ---------------------------------
    ('wp_ds_seam.first', 'conv_c3c1<64,ds,wp>', 'lc', 'r101_1024_b2', 'layer1.0.ds+c3c1', SEAM(2, 256, 256, 64, 64), _L2),
    ('wp_ds_seam.largest', 'conv_c3c1<64,ds,wp>', 'lc', 'ms1697_b16', 'layer1.0.ds+c3c1', SEAM(16, 425, 425, 64, 64), _L2),
    ('wp_ds_seam.walk_even', 'conv_c3c1<64,ds,wp>', 'lc', 'ms1697_b1', 'layer1.0.ds+c3c1', SEAM(1, 425, 425, 64, 64), _L2),
    ('wp_ds_seam.one', 'conv_c3c1<64,ds,wp>', 'lc', 'synthetic', 'test_downsample_seam_roles_split', SEAM(3, 37, 41, 64, 64), _L2),
    # ---- conv_igemm<64x256_wregd1x1/dual>: layer2.0's conv3 + downsample, weights in registers ---------------------------------------
    ('wregd.first', 'conv_igemm<64x256_wregd1x1/dual>', None, 'r101_1024_b2', 'layer2.0.ds+conv3',
     (2, 128, 128, 128, 256, 256, 256, 2, 512, True), _L1),                                                          # 1024 / 256
    ('wregd.largest', 'conv_igemm<64x256_wregd1x1/dual>', None, 'ms1697_b16', 'layer2.0.ds+conv3',
     (16, 213, 213, 128, 256, 425, 425, 2, 512, True), _L1),                                                         # 22686, walk
    ('wregd.one', 'conv_igemm<64x256_wregd1x1/dual>', None, 'synthetic', 'DUAL_SHAPES',
     (2, 13, 11, 128, 256, 26, 21, 2, 512, True), _L1),
    # ---- conv_igemm<256x256_persist1x1_x3/dual>: layers 3-4 (stride-2 source), layer1 below the seam (stride 1) ----------------------
    ('x3dual.first_l3', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride2', 'r101_1024_b3', 'layer3.0.ds+conv3',
     (3, 64, 64, 256, 512, 128, 128, 2, 1024, True), _L1),                                                           # 192: one
    ('x3dual.first_l4', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride2', 'r101_1024_b6', 'layer4.0.ds+conv3',
     (6, 32, 32, 512, 1024, 64, 64, 2, 2048, True), _L1),                                                            # 192: one
    ('x3dual.largest', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride2', 'ms1697_b16', 'layer3.0.ds+conv3',
     (16, 107, 107, 256, 512, 213, 213, 2, 1024, True), _L1),                                                        # 2864, walk
    ('x3dual.walk_l4', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride2', 'ms1697_b16', 'layer4.0.ds+conv3',
     (16, 54, 54, 512, 1024, 107, 107, 2, 2048, True), _L1),                                                         # 1464 / 256
    ('x3dual.walk_b32', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride2', 'r101_1024_b32', 'layer3.0.ds+conv3',
     (32, 64, 64, 256, 512, 128, 128, 2, 1024, True), _L2),                                                          # 2048: 8 each
    ('x3dual_s1.first', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride1', 'native_1023x767', 'layer1.0.ds+conv3',
     (1, 256, 192, 64, 64, 256, 192, 1, 256, True), _L1),                                                            # 192: one
    ('x3dual_s1.largest', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride1', 'ms1200_b1', 'layer1.0.ds+conv3',
     (1, 300, 300, 64, 64, 300, 300, 1, 256, True), _L1),                                                            # 352 / 256
    ('x3dual_s1.walk', 'conv_igemm<256x256_persist1x1_x3/dual>', 'ds_stride1', 'synthetic', '',
     (3, 300, 301, 64, 64, 300, 301, 1, 256, True), _L1),                                                            # 1059 / 256
    # ---- conv_pair: fp16p's paired 1x1 convs of layer1 without a seam (one workgroup per 128 x 128 / 128 x 64 tile) -------------------
    ('pair_xw64.first', 'conv_pair<128x64_xw>', None, 'native_500x375', 'layer1.0.conv1', (1, 125, 94, 64, 64, 1, 1, False, True), _L2),
    ('pair_xw64.largest', 'conv_pair<128x64_xw>', None, 'ms1697_b16', 'layer1.0.conv1', (16, 425, 425, 64, 64, 1, 1, False, True), _L2),
    ('pair_xw128.first', 'conv_pair<128x128_xw>', None, 'native_500x375', 'layer1.0.downsample', (1, 125, 94, 64, 256, 1, 1, False, False), _L2),
    ('pair_xw128.largest', 'conv_pair<128x128_xw>', None, 'ms1200_b1', 'layer1.0.downsample', (1, 300, 300, 64, 256, 1, 1, False, False), _L2),
    ('pair_w128.first', 'conv_pair<128x128_w>', None, 'native_500x375', 'layer1.1.conv3', (1, 125, 94, 64, 256, 1, 1, True, True), _L2),
    ('pair_w128.largest', 'conv_pair<128x128_w>', None, 'ms1200_b1', 'layer1.1.conv3', (1, 300, 300, 64, 256, 1, 1, True, True), _L2),
    ('pair_w64.first', 'conv_pair<128x64_w>', None, 'native_500x375', 'layer1.1.conv1', (1, 125, 94, 256, 64, 1, 1, False, True), _L2),
    ('pair_w64.largest', 'conv_pair<128x64_w>', None, 'ms1200_b1', 'layer1.1.conv1', (1, 300, 300, 256, 64, 1, 1, False, True), _L2),
    # ---- stems --------------------------------------------------------------------------------------------------------------------
    ('stem_u8_raw.first', 'stem_pool_u8', 'raw', 'r50_224_b64', 'conv1+maxpool', STEM(64, 224, 224), _L2),        # 1024 / 512
    ('stem_u8_raw.largest', 'stem_pool_u8', 'raw', 'r101_1024_b32', 'conv1+maxpool', STEM(32, 1024, 1024), _L2),  # 5184: walk
    ('stem_u8_raw.one', 'stem_pool_u8', 'raw', 'synthetic', 'test_stem_u8_gpu.SIZES', STEM(2, 64, 96), _L2),
    ('stem_u8_prep.first', 'stem_pool_u8', 'prep', 'native_500x375', 'conv1+maxpool', STEM(1, 500, 375), _L2),    # 294: one
    ('stem_u8_prep.largest', 'stem_pool_u8', 'prep', 'ms1697_b16', 'conv1+maxpool', STEM(16, 1697, 1697), _L2),   # 6496: walk
    ('stem_pair_walk.first', 'stem_pool_pair', 'walk', 'r50_224_b64', 'conv1+maxpool', STEM(64, 224, 224), _L2),
    ('stem_pair_walk.largest', 'stem_pool_pair', 'walk', 'r101_1024_b32', 'conv1+maxpool', STEM(32, 1024, 1024), _L2),
    ('stem_pair_walk.one', 'stem_pool_pair', 'walk', 'synthetic', 'test_stem_pool_pair_vs_torch_fp32', STEM(2, 64, 96), _L2),
    ('stem_pair_2k.first', 'stem_pool_pair', 'twokernel', 'native_500x375', 'conv1+maxpool', STEM(1, 500, 375), _L2),
    ('stem_pair_2k.largest', 'stem_pool_pair', 'twokernel', 'ms1697_b16', 'conv1+maxpool', STEM(16, 1697, 1697), _L2),
    ('stem_pool.first', 'stem_pool', 'persist', 'native_500x375', 'conv1+maxpool', STEM(1, 500, 375), _L1),      # 294: one
    ('stem_pool.largest', 'stem_pool', 'persist', 'ms1697_b16', 'conv1+maxpool', STEM(16, 1697, 1697), _L1),     # 65888: walk
]


def form_of(row):
    return row[1], row[2]


def table_problems(cases=None):
    """What the table lacks or gets wrong against the mirror and the launch geometry: a list of messages (empty = in step).
    Every mirrored form needs rows in each regime - first / largest at the smallest / largest work-unit count among its claimed
    launches, walk (persistent forms) and one by launch_geometry, and for the role-split DS seam (whose counted pair loop stores an
    odd last tile twice) walks with an odd and an even tile count on the first workgroup; every row with a workload must be that
    workload's launch of the form, with the operands of that layer."""
    cases = ENGINE_CASES if cases is None else cases
    launches = all_launches()
    out = []
    tags = [r[0] for r in cases]
    out += ['tag %s is not unique' % t for t in sorted({t for t in tags if tags.count(t) > 1})]
    for r in cases:
        tag, label, sub, wl, rec, shape, dtypes = r
        form = form_of(r)
        if form not in launches:
            out.append('%s: %s is not a form the engine launches on the claimed workloads' % (tag, form))
            continue
        if len(shape) != len(SHAPE_FIELDS[family(label)]):
            out.append('%s: shape %s does not have the fields %s' % (tag, shape, SHAPE_FIELDS[family(label)]))
            continue
        if wl == 'synthetic':
            continue
        where = {(w, rc) for w, rc, _, _ in launches[form]}
        if (wl, rec) not in where:
            out.append('%s: the engine does not launch %s at %s %s' % (tag, form, wl, rec))
        elif tuple(shape) != layer_shape(wl, rec, label):
            out.append('%s: shape %s is not %s %s (%s)' % (tag, shape, wl, rec, layer_shape(wl, rec, label)))
        bad = set(dtypes) - {d for w, rc, d, _ in launches[form] if (w, rc) == (wl, rec)}
        if bad:
            out.append('%s: the engine does not launch it in %s' % (tag, sorted(bad)))
    for form, ls in sorted(launches.items(), key=str):
        rows = [r for r in cases if form_of(r) == form]
        lo, hi = form_extremes(form, ls)
        real = [launch_geometry(form, r[5])[0] for r in rows if r[3] != 'synthetic']
        need = {'first': lo in real, 'largest': hi in real, 'one': any('one' in regimes(form, r[5]) for r in rows)}
        if walks(form):
            need['walk'] = any('walk' in regimes(form, r[5]) for r in rows)
        if form[1] == 'lc':
            par = {_cdiv(*launch_geometry(form, r[5])[:2]) % 2 for r in rows if 'walk' in regimes(form, r[5])}
            need['walk, odd tiles per workgroup'] = 1 in par
            need['walk, even tiles per workgroup'] = 0 in par
        out += ['%s %s: no row in the %s regime%s' % (form[0], form[1] or '', k, ' (%d work units)' % (lo if k == 'first' else hi)
                                                     if k in ('first', 'largest') else '') for k, ok in need.items() if not ok]
    return out

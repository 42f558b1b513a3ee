"""The fp16 overflow word (csrc/dir_common.h Ovf), kernel by kernel and store form by store form.

Every per-op launch here runs under ops.overflow_watch(), which attaches a device word to the per-op entry points the way an
engine attaches its own.  The operands come from tests/overflow_plant.py: the random operands of the parity tests, clean or
with one product of 2^18 planted at a chosen output (m, n); tests/test_overflow_plant_cpu.py proves on the CPU that the fp32
reference of those operands is non-finite in fp16 exactly there.  What is asserted, always exactly:

  * fp16: the WHOLE word - 0 when the reference stores nothing non-finite, 1 when it does (a spin-limit report, bit 1, fails
    either) - and the kernel's own output: its non-finite positions equal the reference's;
  * bf16: the same plants give word 0 and finite outputs.

A test item is one shape (or one entry point) and walks its variants, forms and dtypes itself - thousands of launches cost
seconds, thousands of test items would cost more than that in set-up alone.  Every variant / form / dtype is still judged: a
failed one is recorded and the walk goes on, and the item fails at its end with one line per failure, each naming the entry
point, the variant or form, the dtype, the plant and the word."""
import pytest
import torch

import overflow_plant as P
from test_ops_gpu import CONV_CASES, CONV_SHAPES, DTYPES, DUAL_SHAPES, SEAM_SHAPES, SPLITK_SHAPES, _variant_names, variant_admissible

pytestmark = pytest.mark.gpu

SPLITK_VARIANTS = ['128x128_w2x2', '64x128_w2x2']
KSPLITS = [2, 3, -1]
BOTH = ['bf16', 'fp16']


def _ops():
    from dirtorch_amd import ops
    return ops


def _dev(case):
    return {k: (v.cuda() if v is not None else None) for k, v in case.items()}


class Failures(list):
    """Runs the steps of one test item; an AssertionError of a step is kept (its first line) and the next step still runs.
    Anything else - a library error, a device fault - ends the item at once."""

    def run(self, step, *args, **kwargs):
        try:
            step(*args, **kwargs)
        except AssertionError as e:
            self.append(str(e).split('\n')[0][:600])

    def done(self):
        assert not self, '%d failed:\n%s' % (len(self), '\n'.join(self))


def _check(watch, outputs, expected, dname, what, judged=None):
    """outputs / expected: one tensor and one set, or matching tuples.  Reads (and clears) the word, which every expected set
    decides; judged: how many of the outputs are compared with their sets (default: all)."""
    word = watch.read()
    outputs = outputs if isinstance(outputs, (tuple, list)) else (outputs,)
    expected = expected if isinstance(expected, (tuple, list)) else (expected,)
    if dname != 'fp16':
        expected = tuple(frozenset() for _ in expected)
    want_word = 1 if any(expected) else 0
    outputs, expected = outputs[:judged], expected[:judged]
    got = tuple(P.nonfinite(o) for o in outputs)
    assert word == want_word and got == tuple(expected), (
        '%s %s: overflow word %d (want %d); non-finite outputs %s, the reference has %s'
        % (what, dname, word, want_word, [sorted(g)[:6] for g in got], [sorted(e)[:6] for e in expected]))


# ---- a-c: the plain convolution, every admissible (shape, variant) pair ------------------------------------------------------
def _conv_launch(ops, shape, dev, variant=-1, ksplit=None, naive=False, relu=None):
    y = ops.conv_bn_act(dev['x'], dev['w'], dev['bias'], dev['res'], stride=shape[7], pad=shape[8],
                        relu=shape[10] if relu is None else relu, variant=variant, ksplit=ksplit, naive=naive)
    if ksplit is not None and ops.conv_bn_act.last_ksplit < 2:
        raise RuntimeError('%s: a split-K launch that did not split' % shape[0])
    return y


def _conv_expected(ops, shape, name, dname, dev, edits):
    """The reference's non-finite set: the CPU's where it is affordable, else the library's plain device checker's (same operands)"""
    if dname != 'fp16':
        return frozenset()
    if P.small(shape):
        return P.conv_expected(name, dname, tuple(edits))
    return P.nonfinite(_conv_launch(ops, shape, dev, naive=True))


def _conv_run(fails, shape, name, dname, launches):
    """launches: [(label, keyword arguments of the launch)].  One upload of the operands, edited in place on the device: the clean
    launch, the single plants and the cancelling pairs, each through every launch of the list."""
    ops = _ops()
    dev = _dev(P.conv_case(name, dname))
    plants = [('clean', (), frozenset())]
    plants += [('plant (m, n) = (%d, %d) sign %+d' % (m, n, sign), edits, intended) for m, n, sign, edits, intended in P.conv_plants(shape)]
    plants += [('cancelling pair at (m, n) = (%d, %d)' % (m, n), tuple(P.conv_cancelling(shape, m, n)), frozenset())
               for m, n in P.conv_cancel_positions(shape)]
    with ops.overflow_watch() as watch:
        for label, edits, intended in plants:
            undo = P.plant_on_device(dev, edits)
            want = _conv_expected(ops, shape, name, dname, dev, edits)
            fails.run(_same, want, intended if dname == 'fp16' else frozenset(), name, label)
            watch.read()      # (the device checker does not report, and must not have)
            for what, kw in launches:
                fails.run(_check, watch, _conv_launch(ops, shape, dev, **kw), want, dname, 'dir_conv_bn_act %s %s %s' % (name, what, label))
            P.plant_on_device(dev, undo)


def _same(want, intended, name, label):
    assert want == intended, 'the reference of %s %s is non-finite at %s, the plant intends %s' % (name, label, sorted(want)[:6], sorted(intended))


ROWS = [s for s in CONV_SHAPES if any(c[0] is s for c in CONV_CASES)]


def test_the_matrix_is_the_parity_matrix():
    assert len(ROWS) == len(CONV_SHAPES) and sum(1 for s, v in CONV_CASES) > 100


@pytest.mark.parametrize('shape', ROWS, ids=[s[0] for s in ROWS])
def test_conv_variant_word_clean_planted_and_cancelling(shape):
    """Every admissible variant of the row, bf16 and fp16.  (a) clean operands: word 0.  (b) one product of +-2^18 at the four
    corners of the [M, Cout] output and one interior element, -1024 too at (0, 0): word 1 and the kernel's output non-finite exactly
    where the reference's is - nothing for -1024 under a ReLU.  '3x3_s2_persistent' (288 tiles) plants in the first and the last
    tile a persistent workgroup walks.  (c) +2^18 and -2^18 into one output: partial sums above the range, a finite sum, word 0."""
    names = _ops().conv_variant_names()
    launches = [('variant %s' % v, dict(variant=names.index(v))) for s, v in CONV_CASES if s is shape]
    fails = Failures()
    for dname in BOTH:
        _conv_run(fails, shape, shape[0], dname, launches)
    fails.done()


@pytest.mark.parametrize('shape', SPLITK_SHAPES, ids=[s[0] for s in SPLITK_SHAPES])
def test_splitk_word_comes_from_the_reduce_kernel(shape):
    """(e) ksplit 2, 3 and the library's own choice on both split-K variants.  The main kernel writes fp32 partials, which are
    never judged; the reduce kernel packs and reports.  The cancelling pair at (0, 0) puts +2^18 and -2^18 into different K slices
    wherever the slices separate channel 0 from the last 64 (ksplit 2 on every row, any ksplit on the 1x1 rows): the partials are
    out of range, the sum is not."""
    ops = _ops()
    names = ops.conv_variant_names()
    launches = [('variant %s split-K %d' % (v, ks), dict(variant=names.index(v), ksplit=ks)) for v in SPLITK_VARIANTS for ks in KSPLITS]
    fails = Failures()
    for dname in BOTH:
        _conv_run(fails, shape, 'splitk/' + shape[0], dname, launches)
    fails.done()


# ---- b, continued: persistent kernels where every workgroup walks several tiles -------------------------------------------------
# (name, B, H, W, Cin, Cout, k, stride, pad, residual, relu): more tiles than the kernels below have workgroups (one or two per
# CU, 256 CUs) - 268 tiles of 256 x 256, 536 of 64 x 512, 4288 of 64 x 64; 280 patches of 8 x 32 pixels, 1120 tiles of 64 x 64
WALK_SHAPES = [
    ('1x1_res_k128_n1024', 2, 92, 93, 128, 1024, 1, 1, 0, True, True),
    ('1x1_k256_n1024', 2, 92, 93, 256, 1024, 1, 1, 0, False, True),
    ('3x3_c64', 5, 64, 224, 64, 64, 3, 1, 1, False, True),
]
WALKERS = ('persist1x1', 'lc1x1', 'wreg1x1', 'ring1x1', 'small_s', 'patchlc3x3')      # the kernels with a tile loop
WALK_CASES = [(s, v) for s in WALK_SHAPES for v in _variant_names() if any(k in v for k in WALKERS)
              and variant_admissible(v, s[4], s[5], s[6], s[7], s[8], s[9])]


def test_the_tile_walking_kernels_are_all_in_the_matrix():
    have = set(v for s, v in WALK_CASES)
    assert have >= {'256x256_persist1x1', '256x256_persist1x1_x3', '256x256_lc1x1', '64x512_wreg1x1', '64x64_small_s8', '64x64_small_s4',
                    '64x64_small_s4k2', '256x64_patchlc3x3'}, have


@pytest.mark.parametrize('shape', WALK_SHAPES, ids=[s[0] for s in WALK_SHAPES])
def test_persistent_kernels_report_from_every_tile_they_walk(shape):
    """A tracker declared inside the tile loop would report only the last tile a workgroup walks: plants in the first tile, the
    last (ragged) one and the middle, one launch each, fp16.  Operands are made on the device; the expected set is the library's
    plain device checker's and must be the singleton (nothing for -1024 under the ReLU)."""
    ops = _ops()
    names = ops.conv_variant_names()
    name, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    M = P.geom(shape)[12]
    g = torch.Generator(device='cuda').manual_seed(53)
    r = lambda *sh: torch.randn(*sh, generator=g, device='cuda')      # noqa: E731
    dev = {'x': r(B, H, W, Cin).half(), 'w': (r(Cout, k, k, Cin) * (2.0 / (k * k * Cin)) ** 0.5).half(), 'bias': r(Cout) * 0.2,
           'res': r(B, H, W, Cout).half() if use_res else None}
    variants = [v for s, v in WALK_CASES if s is shape]
    fails = Failures()
    with ops.overflow_watch() as watch:
        for label, edits, intended in [('clean', (), frozenset())] + [
                ('plant (m, n) = (%d, %d) of M = %d, sign %+d' % (m, n, M, sign), e, i) for m, n, sign, e, i in P.conv_plants(shape)]:
            undo = P.plant_on_device(dev, edits)
            assert P.nonfinite(_conv_launch(ops, shape, dev, naive=True)) == intended, (name, label)
            watch.read()
            for v in variants:
                fails.run(_check, watch, _conv_launch(ops, shape, dev, variant=names.index(v)), intended, 'fp16',
                          'dir_conv_bn_act %s variant %s %s' % (name, v, label))
            P.plant_on_device(dev, undo)
    fails.done()


# ---- d: the boundary of the format --------------------------------------------------------------------------------------------
def _first_small_row(vname):
    for s, v in CONV_CASES:
        if v == vname and P.small(s):
            return s
    return None


BOUNDARY_VARIANTS = sorted(set(v for s, v in CONV_CASES if P.small(s)))


def _boundary(watch, ops, vname):
    shape = _first_small_row(vname)
    variant = ops.conv_variant_names().index(vname)
    M, Cout = P.geom(shape)[12], shape[5]
    m, n = P.positions(M, Cout)[4]
    for bias_n, value, word in ((15.0, P.F16_MAX, 0), (16.0, float('inf'), 1)):
        y = _conv_launch(ops, shape, _dev(P.conv_boundary(shape, m, n, bias_n)), variant=variant, relu=False)
        got = watch.read()
        y = y.float().cpu().reshape(M, Cout)
        what = 'dir_conv_bn_act %s variant %s fp16 boundary bias %g at (m, n) = (%d, %d): word %d (want %d), y %r (want %r)' % (
            shape[0], vname, bias_n, m, n, got, word, float(y[m, n]), value)
        assert got == word and float(y[m, n]) == value, what
        y[m, n] = bias_n
        assert bool((y[:, n] == bias_n).all()) and float(y.abs().sum()) == bias_n * M, what


def test_boundary_65519_is_stored_finite_and_65520_is_flagged():
    """y[m, n] = 65504 + bias exactly: 65519 rounds to 65504 (word 0), 65520 is the tie that rounds to inf (word 1).  Every
    variant of the table, on its first admissible small row."""
    assert set(BOUNDARY_VARIANTS) == set(v for s, v in CONV_CASES)
    ops = _ops()
    fails = Failures()
    with ops.overflow_watch() as watch:
        for vname in BOUNDARY_VARIANTS:
            fails.run(_boundary, watch, ops, vname)
            watch.read()
    fails.done()


# ---- f: the fused seams ---------------------------------------------------------------------------------------------------------
def _seam_launch(ops, entry, dev, relu3, keep_stride=0):
    """-> (y, t1); with a keep_stride, y is pre-filled with zeros so that the pixels the kernel leaves alone are finite"""
    wp = lambda k: (dev[k], dev.get(k + '_lo'))      # noqa: E731
    y0 = torch.zeros_like(dev['res']) if 'res' in dev else None
    if entry == 'conv_c3c1':
        return ops.conv_c3c1(dev['t2'], dev['w3'], dev['b3'], dev['res'], dev['w1'], dev['b1'], relu3=relu3)
    if entry == 'conv_c3c1_keep':
        return ops.conv_c3c1_keep(dev['t2'], dev['w3'], dev['b3'], dev['res'], dev['w1'], dev['b1'], keep_stride=keep_stride, y=y0, relu3=relu3)
    if entry == 'conv_c3c1_ds':
        return ops.conv_c3c1_ds(dev['t2'], dev['x'], dev['w3'], dev['b3'], dev['w1'], dev['b1'], relu3=relu3)
    if entry == 'conv_c3c1_wpair':
        return ops.conv_c3c1_wpair(dev['t2'], wp('w3'), dev['b3'], dev['res'], wp('w1'), dev['b1'], relu3=relu3)
    if entry == 'conv_c3c1_wpair_keep':
        return ops.conv_c3c1_wpair_keep(dev['t2'], wp('w3'), dev['b3'], dev['res'], wp('w1'), dev['b1'], keep_stride=keep_stride, y=y0, relu3=relu3)
    assert entry == 'conv_c3c1_ds_wpair'
    return ops.conv_c3c1_ds_wpair(dev['t2'], wp('x'), wp('w3'), dev['b3'], wp('w1'), dev['b1'], relu3=relu3)


def _seam_run(fails, form, B, H, W, P1, P2, dname, launches):
    """launches: [(entry point, keep_stride, label suffix)], each run with relu3 on and off on every plant"""
    ops = _ops()
    key = (B, H, W, P1, P2, dname, form)
    case = P.seam_case(*key)
    dev = _dev(case)
    M = B * H * W
    plants = [('clean', [])]
    # y: pixel 0 (stored at a stage exit), pixel 1 = (0, 0, 1) (skipped there - conv1 still consumes it) and the last pixel of the
    # last, ragged tile; -1024 under a ReLU is clamped before the pack.  t1 alone, with y finite: first and last tile.
    for m, n in ((0, 0), (1, 4 * P1 - 1), (M - 1, 2 * P1 + 1)):
        plants.append(('y (m, n) = (%d, %d)' % (m, n), P.seam_plant_y(case, m, n)))
    plants.append(('y (m, n) = (0, 0) sign -1', P.seam_plant_y(case, 0, 0, -1)))
    for m, n2 in ((M - 1, P2 - 1), (0, P2 // 2 + 1)):
        plants.append(('t1 (m, n2) = (%d, %d)' % (m, n2), P.seam_plant_t1(case, m, n2)))
    with ops.overflow_watch() as watch:
        for label, edits in plants:
            undo = P.plant_on_device(dev, edits)
            # With paired conv1 weights an inf in y meets TWO products per output, w1_hi * inf + w1_lo * inf: where their signs differ
            # that is NaN, which conv1's ReLU (a hardware max) turns into 0, while the reference's (w1_hi + w1_lo) * inf stays +-inf.
            # What t1 holds downstream of an overflow that is already stored - and flagged - is not defined; y and the word are.
            judged = 1 if 'w1_lo' in case and label.startswith('y ') else None
            for relu3 in (True, False):
                for entry, keep_stride, suffix in launches:
                    want = P.seam_expected_of(key, edits, relu3, keep_stride) if dname == 'fp16' else (frozenset(), frozenset())
                    what = 'dir_%s%s %dx%dx%d planes %d->%d relu3=%d keep_stride=%d plant %s' % (
                        entry, suffix, B, H, W, P1, P2, relu3, keep_stride, label)
                    fails.run(_check, watch, _seam_launch(ops, entry, dev, relu3, keep_stride), want, dname, what, judged)
            P.plant_on_device(dev, undo)


@pytest.mark.parametrize('B,H,W', SEAM_SHAPES)
def test_seam_word(B, H, W):
    """dir_conv_c3c1 and dir_conv_c3c1_keep (every pixel stored, and a stage exit's keep_stride = 2), planes 64, 128 and 64 -> 128,
    bf16 and fp16, relu3 on and off: both stores report - the block output y and the next conv1's t1 - on a ragged tile set, 400
    tiles on 256 workgroups and a single partial tile."""
    fails = Failures()
    launches = [('conv_c3c1', 0, ''), ('conv_c3c1_keep', 2, ''), ('conv_c3c1_keep', 0, '')]
    for P1, P2 in P.SEAM_PLANES:
        for dname in BOTH:
            _seam_run(fails, 'plain', B, H, W, P1, P2, dname, launches)
    fails.done()


@pytest.mark.parametrize('B,H,W', SEAM_SHAPES)
def test_downsample_seam_word(B, H, W, monkeypatch):
    """dir_conv_c3c1_ds: the loader / consumer kernel (conv_c3c1lc.hip, the default) and conv_c3c1.hip's one-role DS form"""
    fails = Failures()
    for dname in BOTH:
        _seam_run(fails, 'ds', B, H, W, 64, 64, dname, [('conv_c3c1_ds', 0, '')])
    monkeypatch.setenv('DIRTORCH_AMD_NO_C3C1LC', '1')
    for dname in BOTH:
        _seam_run(fails, 'ds', B, H, W, 64, 64, dname, [('conv_c3c1_ds', 0, ' (NO_C3C1LC)')])
    fails.done()


@pytest.mark.parametrize('B,H,W', SEAM_SHAPES)
def test_paired_weight_seam_word(B, H, W, monkeypatch):
    """dir_conv_c3c1_wpair, _wpair_keep (P2 = 64 and 128) and _ds_wpair, in both wave-role forms: fp16 with (hi, lo) weight planes"""
    fails = Failures()
    for P2 in (64, 128):
        _seam_run(fails, 'wp', B, H, W, 64, P2, 'fp16', [('conv_c3c1_wpair', 0, ''), ('conv_c3c1_wpair_keep', 2, '')])
    _seam_run(fails, 'ds_wp', B, H, W, 64, 64, 'fp16', [('conv_c3c1_ds_wpair', 0, '')])
    monkeypatch.setenv('DIRTORCH_AMD_NO_C3C1LC', '1')
    _seam_run(fails, 'ds_wp', B, H, W, 64, 64, 'fp16', [('conv_c3c1_ds_wpair', 0, ' (NO_C3C1LC)')])
    fails.done()


@pytest.mark.parametrize('B,H,W', [(1, 8, 8), (4, 80, 80)])
@pytest.mark.experiments      # conv_seam3.hip ships in experiments builds only (DIR_EXPERIMENTS=1 csrc/build.sh)
def test_layer3_seam_word(B, H, W):
    """planes 256 (conv_seam3.hip): whole 64-pixel tiles only"""
    fails = Failures()
    for dname in BOTH:
        _seam_run(fails, 'plain', B, H, W, 256, 256, dname, [('conv_c3c1', 0, '')])
    fails.done()


# ---- g: the two-source GEMM, the paired forms, the stems, upsample_add --------------------------------------------------------
def _dual_run(fails, shape, dname, what):
    ops = _ops()
    B, OH, OW, Cin, Cout, Cin2, s2 = shape
    case = P.dual_case(*shape, dname)
    dev = _dev(case)
    plants = [('clean', [], True)]
    for i, (m, n) in enumerate(P.positions(B * OH * OW, Cout)):
        plants.append(('(m, n) = (%d, %d) source %d' % (m, n, i % 2), P.dual_plant(case, s2, m, n, i % 2), True))
    plants.append(('(m, n) = (0, 0) source 1 sign -1', P.dual_plant(case, s2, 0, 0, 1, -1), True))
    plants.append(('(m, n) = (0, 0) source 1 sign -1, no ReLU', P.dual_plant(case, s2, 0, 0, 1, -1), False))
    plants.append(('cancelling pair at the last element', P.dual_cancelling(case, s2, B * OH * OW - 1, Cout - 1), True))
    with ops.overflow_watch() as watch:
        for label, edits, relu in plants:
            want = P.dual_expected_of(shape + (dname,), edits, s2, relu)
            undo = P.plant_on_device(dev, edits)
            y = ops.conv_dual(dev['t2'], dev['x'], dev['wcat'], dev['bias'], stride2=s2, relu=relu)
            fails.run(_check, watch, y, want, dname, 'dir_conv_dual %s %s plant %s' % (shape, what, label))
            P.plant_on_device(dev, undo)


@pytest.mark.parametrize('shape', DUAL_SHAPES, ids=['%dx%dx%d-%d-%d-%d-s%d' % s for s in DUAL_SHAPES])
def test_two_source_gemm_word(shape, monkeypatch):
    """dir_conv_dual through either source, bf16 and fp16: the default pick (layer2's shape: conv_wregd.hip), conv_persist.hip's
    DUAL ring (DIRTORCH_AMD_NO_WREGD) and the loader / consumer ring conv_persistlc.hip (DIRTORCH_AMD_LC1X1)"""
    fails = Failures()
    for what, switch in (('default', None), ('NO_WREGD', 'NO_WREGD'), ('NO_WREGD LC1X1', 'LC1X1')):
        if switch:
            monkeypatch.setenv('DIRTORCH_AMD_' + switch, '1')
        for dname in BOTH:
            _dual_run(fails, shape, dname, what)
    fails.done()


def test_two_source_gemm_word_where_workgroups_walk_several_tiles(monkeypatch):
    """layer2.0's shape at 34560 pixels: 540 tiles of 64 pixels on conv_wregd.hip's 128 workgroups per channel slice, 270 tiles of
    256 x 256 on the 256 workgroups of the DUAL ring and of its loader / consumer form.  Reference: fp32 matrix products of the same
    operands on the device."""
    ops = _ops()
    B, OH, OW, Cin, Cout, Cin2, s2 = 4, 96, 90, 128, 512, 256, 2
    g = torch.Generator(device='cuda').manual_seed(59)
    r = lambda *sh: torch.randn(*sh, generator=g, device='cuda')      # noqa: E731
    dev = {'t2': r(B, OH, OW, Cin).relu().half(), 'x': r(B, 2 * OH, 2 * OW - 1, Cin2).relu().half(),
           'wcat': torch.cat([r(Cout, Cin) * (2.0 / Cin) ** 0.5, r(Cout, Cin2) * (2.0 / Cin2) ** 0.5], dim=1).half().contiguous(), 'bias': r(Cout) * 0.3}
    M = B * OH * OW

    def reference():
        rows = torch.cat([dev['t2'].reshape(M, Cin), dev['x'][:, ::s2, ::s2][:, :OH, :OW].reshape(M, Cin2)], dim=1).float()
        return P.nonfinite(torch.relu(rows @ dev['wcat'].float().T + dev['bias']).half())
    plants = [('clean', [], frozenset())]
    for i, (m, n) in enumerate(P.positions(M, Cout)):
        plants.append(('(m, n) = (%d, %d) of M = %d, source %d' % (m, n, M, i % 2), P.dual_plant(dev, s2, m, n, i % 2), frozenset([(m, n)])))
    plants.append(('(m, n) = (0, 0) source 0 sign -1', P.dual_plant(dev, s2, 0, 0, 0, -1), frozenset()))
    fails = Failures()
    for switches in ((), ('NO_WREGD',), ('NO_WREGD', 'LC1X1')):
        for sw in switches:
            monkeypatch.setenv('DIRTORCH_AMD_' + sw, '1')
        with ops.overflow_watch() as watch:
            for label, edits, intended in plants:
                undo = P.plant_on_device(dev, edits)
                assert reference() == intended, label
                y = ops.conv_dual(dev['t2'], dev['x'], dev['wcat'], dev['bias'], stride2=s2, relu=True)
                fails.run(_check, watch, y, intended, 'fp16', 'dir_conv_dual layer2.0 x %d pixels %s plant %s' % (M, switches, label))
                P.plant_on_device(dev, undo)
    fails.done()


def _pair(dev, k):
    return dev[k + '_hi'], dev.get(k + '_lo')


def _pair_cases():
    """test_pair_gpu's geometries; the patch-pair kernel's shapes also on the implicit-GEMM form (DIRTORCH_AMD_NO_PAIR_PATCH)"""
    from test_pair_gpu import GEOMS
    return [(g, False) for g in GEOMS] + [(g, True) for g in GEOMS if g[3:6] == (64, 64, 3) and not g[8]]


def test_paired_conv_word(monkeypatch):
    """dir_conv_bn_act_pair: the plant is in the hi planes and the word is judged on y_hi (y_lo = fp16(y - y_hi) follows it)"""
    ops = _ops()
    fails = Failures()
    for geom, no_patch in _pair_cases():
        B, H, W, Cin, Cout, k, stride, pad, with_res, relu = geom
        if no_patch:
            monkeypatch.setenv('DIRTORCH_AMD_NO_PAIR_PATCH', '1')
        M = B * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
        case = P.pair_case(geom)
        dev = _dev(case)
        plants = [('clean', [])] + [('(m, n) = (%d, %d)' % (m, n), P.pair_plant(geom, m, n)) for m, n in P.positions(M, Cout)]
        plants.append(('(m, n) = (0, 0) sign -1', P.pair_plant(geom, 0, 0, -1)))
        with ops.overflow_watch() as watch:
            for label, edits in plants:
                want = P.pair_expected(geom, P.planted(case, edits))
                undo = P.plant_on_device(dev, edits)
                for pair_out in (True, False):
                    y = ops.conv_bn_act_pair(_pair(dev, 'x'), _pair(dev, 'w'), dev['bias'], _pair(dev, 'res') if with_res else None,
                                             stride=stride, pad=pad, relu=relu, pair_out=pair_out)
                    fails.run(_check, watch, y[0], want, 'fp16', 'dir_conv_bn_act_pair %s%s pair_out=%d plant %s' % (
                        geom, ' NO_PAIR_PATCH' if no_patch else '', pair_out, label))
                P.plant_on_device(dev, undo)
    fails.done()


def test_paired_two_source_word():
    ops = _ops()
    fails = Failures()
    for shape in P.PAIR_DUAL_SHAPES:
        B, H, W, C, Cout = shape
        case = P.pair_dual_case(*shape)
        dev = _dev(case)
        plants = [('clean', [])]
        for i, (m, n) in enumerate(P.positions(B * H * W, Cout)):
            plants.append(('(m, n) = (%d, %d) source %d' % (m, n, i % 2), P.pair_dual_plant(case, m, n, i % 2)))
        plants.append(('(m, n) = (0, 0) sign -1', P.pair_dual_plant(case, 0, 0, 0, -1)))
        with ops.overflow_watch() as watch:
            for label, edits in plants:
                want = P.pair_dual_expected(P.planted(case, edits), True)
                undo = P.plant_on_device(dev, edits)
                y = ops.conv_pair_dual(_pair(dev, 't2'), _pair(dev, 'x'), _pair(dev, 'w'), dev['bias'])
                fails.run(_check, watch, y[0], want, 'fp16', 'dir_conv_pair_dual %s plant %s' % (shape, label))
                P.plant_on_device(dev, undo)
    fails.done()


def _stem_plants(H, W):
    """conv pixels: the corners, two interior ones (odd / even rows and columns pool into one to four windows)"""
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return [(0, 0, 0, 0), (1, OH - 1, OW - 1, 63), (1, 5, 4, 33), (0, 4, 5, 7), (0, OH - 1, 0, 62)]


@pytest.mark.parametrize('H,W', P.STEM_SIZES)
def test_stem_pool_word(H, W, monkeypatch):
    """dir_stem_pool, both forms (the persistent one and DIRTORCH_AMD_STEM_V1's), bf16 and fp16: one conv output of 2^18 becomes
    inf in every pooled pixel whose window holds it"""
    ops = _ops()
    case = P.stem_case(H, W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    plants = [('clean', [])] + [('conv pixel %s' % (p,), P.stem_plant(*p)) for p in _stem_plants(H, W)]
    plants.append(('conv pixel (0, 3, 3, 5) sign -1', P.stem_plant(0, 3, 3, 5, sign=-1)))
    fails = Failures()
    for form in ('persistent', 'one_tile_per_workgroup'):
        if form != 'persistent':
            monkeypatch.setenv('DIRTORCH_AMD_STEM_V1', '1')
        with ops.overflow_watch() as watch:
            for dname in BOTH:
                dt = DTYPES[dname]
                for label, edits in plants:
                    c = P.planted(case, edits)
                    y = ops.stem_pool(ops.prep_input(c['img'].cuda(), dt), ops.pack_stem_weight(c['w7'], dt).cuda(), c['bias'].cuda(), (OH, OW))
                    fails.run(_check, watch, y, P.stem_expected(c, dname), dname, 'dir_stem_pool %dx%d %s plant %s' % (H, W, form, label))
    fails.done()


@pytest.mark.parametrize('H,W', P.STEM_SIZES)
def test_stem_pool_pair_word(H, W, monkeypatch):
    ops = _ops()
    case = P.stem_case(H, W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    plants = [('clean', [])] + [('conv pixel %s' % (p,), P.stem_plant(*p)) for p in _stem_plants(H, W)]
    fails = Failures()
    for form in ('default', 'STEM_V1', 'STEM_PAIR_OLD'):
        if form != 'default':
            monkeypatch.setenv('DIRTORCH_AMD_' + form, '1')
        with ops.overflow_watch() as watch:
            for label, edits in plants:
                c = P.planted(case, edits)
                s2d = ops.prep_input_pair(c['img'].cuda())
                wp = ops.split_pair(ops.pack_stem_weight(c['w7'].cuda(), torch.float32))
                y = ops.stem_pool_pair(s2d, wp, c['bias'].cuda(), (OH, OW))
                fails.run(_check, watch, y[0], P.stem_pair_expected(c), 'fp16', 'dir_stem_pool_pair %dx%d %s plant %s' % (H, W, form, label))
        if form != 'default':
            monkeypatch.delenv('DIRTORCH_AMD_' + form)
    fails.done()


@pytest.mark.parametrize('B,H,W', [(2, 40, 52), (1, 41, 53), (2, 74, 82)])
def test_stem_pool_u8_word(B, H, W, monkeypatch):
    """dir_stem_pool_u8: an even width reads the raw image, an odd one (and DIRTORCH_AMD_STEM_U8_PREP) prep_input_u8's plane; one
    8-wave workgroup per CU under DIRTORCH_AMD_STEM_U8_WG8; segments of the kernel's own length and independent tiles"""
    ops = _ops()
    case = P.stem_u8_case(B, H, W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pixels = [(0, 0, 0, 0), (B - 1, OH - 1, OW - 1, 63), (B - 1, 5, 4, 33), (0, 4, 5, 7)]
    plants = [('clean', [])] + [('conv pixel %s' % (p,), P.stem_u8_plant(case, *p)) for p in pixels]
    fails = Failures()
    for form in ('default', 'STEM_U8_PREP', 'STEM_U8_WG8'):
        if form != 'default':
            monkeypatch.setenv('DIRTORCH_AMD_' + form, '1')
        with ops.overflow_watch() as watch:
            for label, edits in plants:
                c = P.planted(case, edits)
                want = P.stem_u8_expected(c)
                for seg in (0, 1):
                    y = ops.stem_pool_u8(c['u8'].cuda(), c['w'], c['scale'], c['bias'], P.U8_MEAN, P.U8_STD, seg_tiles=seg)
                    fails.run(_check, watch, y[0], want, 'fp16', 'dir_stem_pool_u8 %dx%dx%d %s seg_tiles=%d plant %s' % (B, H, W, form, seg, label))
        if form != 'default':
            monkeypatch.delenv('DIRTORCH_AMD_' + form)
    fails.done()


@pytest.mark.parametrize('dname', BOTH)
def test_stem_pool_word_where_workgroups_walk_several_tiles(dname):
    """2 x 1024 x 400: 1204 pooled tiles on 512 persistent workgroups.  Expected: the pool windows of the planted conv pixel,
    which must also be what the library's two-kernel path (conv, then max-pool) stores."""
    ops = _ops()
    dt = DTYPES[dname]
    H, W = 1024, 400
    OH, OW = H // 2, W // 2
    case = P.stem_case(H, W)
    bias = case['bias'].cuda()
    with ops.overflow_watch() as watch:
        for b, oh, ow, n in ((0, 0, 0, 0), (1, OH - 1, OW - 1, 63), (0, 255, 100, 33)):
            c = P.planted(case, P.stem_plant(b, oh, ow, n))
            s2d, wp = ops.prep_input(c['img'].cuda(), dt), ops.pack_stem_weight(c['w7'], dt).cuda()
            want = P.pool_windows(b, oh, ow, n, OH, OW) if dname == 'fp16' else frozenset()
            two = ops.maxpool_3x3s2(ops.conv_bn_act(s2d, wp, bias, None, stride=1, pad=2, relu=True, out_hw=(OH, OW)))
            assert P.nonfinite(two) == want and watch.read() == (1 if want else 0)
            _check(watch, ops.stem_pool(s2d, wp, bias, (OH, OW)), want, dname, 'dir_stem_pool %dx%d plant conv pixel %s' % (H, W, (b, oh, ow, n)))


def test_paired_stems_word_where_workgroups_walk_several_tiles():
    """dir_stem_pool_u8 at 2 x 513 x 640 and dir_stem_pool_pair at 1 x 513 x 767 (the largest sizes of their parity tests), a plant in
    the first and in the last tile; reference in fp32 on the CPU."""
    ops = _ops()
    with ops.overflow_watch() as watch:
        B, H, W = 2, 513, 640
        case = P.stem_u8_case(B, H, W)
        for p in ((0, 0, 0, 0), (B - 1, (H - 1) // 2, (W - 1) // 2, 63)):
            c = P.planted(case, P.stem_u8_plant(case, *p))
            want = P.stem_u8_expected(c, torch.float32)
            assert want == P.pool_windows(*p, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
            y = ops.stem_pool_u8(c['u8'].cuda(), c['w'], c['scale'], c['bias'], P.U8_MEAN, P.U8_STD)
            _check(watch, y[0], want, 'fp16', 'dir_stem_pool_u8 %dx%dx%d plant conv pixel %s' % (B, H, W, p))
        H, W = 513, 767
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        g = torch.Generator().manual_seed(29)
        case = {'img': torch.randn(1, 3, H, W, generator=g), 'w7': torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5, 'bias': 0.3 * torch.randn(64, generator=g)}
        for p in ((0, 0, 0, 0), (0, OH - 1, OW - 1, 63)):
            c = P.planted(case, P.stem_plant(*p))
            want = P.stem_pair_expected(c, torch.float32)
            assert want == P.pool_windows(*p, OH, OW)
            y = ops.stem_pool_pair(ops.prep_input_pair(c['img'].cuda()), ops.split_pair(ops.pack_stem_weight(c['w7'].cuda(), torch.float32)), c['bias'].cuda(), (OH, OW))
            _check(watch, y[0], want, 'fp16', 'dir_stem_pool_pair %dx%d plant conv pixel %s' % (H, W, p))


def test_upsample_add_word():
    ops = _ops()
    fails = Failures()
    for shape in P.UPSAMPLE_SHAPES:
        B, H, W, h, w, C = shape
        for dname in BOTH:
            case = P.upsample_case(*shape, dname)
            dev = _dev(case)
            plants = [('clean', [])] + [('(m, n) = (%d, %d)' % p, P.upsample_plant(case, *p)) for p in P.positions(B * H * W, C)]
            with ops.overflow_watch() as watch:
                for label, edits in plants:
                    want = P.upsample_expected(P.planted(case, edits), dname)
                    undo = P.plant_on_device(dev, edits)
                    fails.run(_check, watch, ops.upsample_add(dev['x'], dev['low']), want, dname, 'dir_upsample_add %s plant %s' % (shape, label))
                    P.plant_on_device(dev, undo)
    fails.done()


# ---- h: the word itself -----------------------------------------------------------------------------------------------------------
def test_word_is_sticky_read_clears_and_the_hook_ends_with_the_block():
    ops = _ops()
    shape = P.SHAPE_BY_NAME['1x1_k256']
    name = shape[0]
    clean = _dev(P.conv_case(name, 'fp16'))
    bad = _dev(P.planted(P.conv_case(name, 'fp16'), P.conv_single(shape, 5, 7)))
    assert P.conv_expected(name, 'fp16', tuple(P.conv_single(shape, 5, 7))) == frozenset([(5, 7)])
    with ops.overflow_watch() as watch:
        assert watch.read() == 0
        _conv_launch(ops, shape, bad)
        _conv_launch(ops, shape, clean)
        assert watch.read() == 1          # sticky across the second, clean launch
        assert watch.read() == 0          # read() cleared it
        _conv_launch(ops, shape, clean)
        assert watch.read() == 0
    # the hook is unset again: a planted launch between two blocks reports nowhere, its output is what it was ...
    y = _conv_launch(ops, shape, bad)
    assert P.nonfinite(y) == frozenset([(5, 7)])
    with ops.overflow_watch() as watch:
        assert watch.read() == 0          # ... and a fresh word starts at 0
        y2 = _conv_launch(ops, shape, bad)
        assert watch.read() == 1
    assert torch.equal(y.view(torch.int16), y2.view(torch.int16))      # the word changes no output bit

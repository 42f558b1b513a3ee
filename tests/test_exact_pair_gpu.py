"""The paired-fp16 kernels of DIR_FP16P, BIT FOR BIT in BOTH planes against fp64 on the CPU, on operands whose fp32 sums are exact
in every order (tests/exact_pair.py: the pair lattice, its bit budget and the references; tests/test_exact_pair_cpu.py checks on
the CPU that the references are exact and that lo planes, every product, the ReLU, a rounding lo and a subnormal lo are exercised
on the rows used here).

tests/test_pair_gpu.py keeps realistic magnitudes and gates the pair kernels at 4e-6 |ref|max (convolutions, stem) and at one
fp16 ulp of the largest output (seams).  A lo-plane product lost for one K step or one filter tap, an output split that truncates,
a residual lo plane added after the ReLU all pass those gates.  Here the expected planes are one pair of bit patterns:

    hi == RNE_fp16(v),  lo == RNE_fp16(v - hi),  v = act(sum(w_hi.x_hi + w_hi.x_lo + w_lo.x_hi) + bias (+ res_hi (+ res_lo)))

with zero tolerance, over all elements, for conv_bn_act_pair (every kernel form test_pair_gpu.GEOMS reaches, x and the residual as
pairs and as single planes, pair_out on and off, a ragged patch row, a row whose lo ROUNDS and a row whose lo is SUBNORMAL),
conv_pair_dual (also against the two launches it replaces), conv_c3c1_wpair and conv_c3c1_ds_wpair (y and t1, both kernels of
the downsample form), stem_pool_pair in its three forms (each against the reference, not only against each other),
prep_input_pair's fp32 feed on arbitrary values, and stem_pool_u8 in its raw / prep / one-workgroup forms and segment lengths.  A
failure names the plane, the first differing (pixel, channel), its tile, both bit patterns and the distance in lattice units.

What the tests see of arithmetic-only mutants (no address, bound, barrier or wait count changed; built into a second library that
was never part of the tree; one run on the MI355X per mutant of this file - 56 cases - and of test_pair_gpu.py's kernel tests;
"share" = differing elements of the first failing comparison).  Every mutant fails here.  test_pair_gpu.py's tolerances catch more
than their width suggests - a lost lo product is ~30 x its 4e-6 gate, not 1 x - but a split that truncates passes them:

  mutant                                            fails here (share)                                  test_pair_gpu.py
  1 conv_pair_kernel: no w_hi.x_lo in K sub-step     conv 14 / 14, dual 3 / 3 (hi 50.6 %, lo 1.1 %)      caught: 4e-6 gate, 11 conv + 3 dual (err
    ks == 1 only                                                                                        8e-4 ... 1e-3 of 2.3e-5 ... 3.2e-5)
  2 conv_pair_patch64_kernel: lo step of tap 8       conv 4 / 14: the four patch rows (hi 36.8 %,        caught: 4e-6 gate on the three patch rows
    skipped                                          lo 26.6 %)                                          (err 2.9e-4 ... 3.7e-4)
  3 split2: lo from a truncated hi, hi rounded       conv 14, dual 3, stem 8 (both conv_pair.hip         caught: 4e-6 gate, 11 conv + 3 dual (err up
                                                     forms), prep 1 (lo 18.3 %)                          to 7.8e-3), prep 2, stem form equality 6
  4 conv_pair_kernel: residual lo plane added        conv 2 / 14: the residual rows, dual 3 / 3: the     caught: 4e-6 gate, 2 conv + the dual's
    after the ReLU                                   two-launch leg (hi 46.7 %)                          two-launch leg 3 (err 1e-3 ... 2e-3)
  5 conv_c3c1 WP1: no w1_lo in K step 1              seam 6 / 8: every paired w1 (t1 48.7 %), ds seam    caught: seam gate 3 (its lo planes are as
                                                     3 / 6: the one-role kernel (t1 54.2 %)              large as hi), roles-split == one-role 3
  6 stem_pool_pair_persist_kernel: no w_lo.x_hi      stem 4 / 12: that form at every size (hi 8.6 %,     caught ONLY kernel against kernel (form
    for filter row R = 3                             lo 66.7 % at 7 x 9)                                 equality 6); the 4e-6 gate sees the default form
  7 split2: hi TRUNCATED, lo from that hi (a         conv 14, dual 3, stem 8, prep 1 (hi 18.3 %,         MISSED by all 11 conv and 3 dual cases; seen
    consistent pair: hi + lo == v still)             lo 18.3 %)                                          only where two kernels meet (prep 2, stem 6)
  8 mutant 6 in ALL THREE stem forms (a mistake      stem 12 / 12 (same shares in every form)            caught: 4e-6 gate 6 (err 5e-4 ... 8e-4 of 2e-5)
    the forms share)
  9 mutant 5 in BOTH downsample-seam kernels         seam 6 / 8, ds seam 6 / 6 (t1 54.2 %)               caught: seam gates 3 + 2 (large lo planes);
                                                                                                         roles-split == one-role passes, 3 / 3
 10 split2: lo truncated to 11 bits, not rounded     conv 1 / 14: the top-binade row alone (lo 11.9 %),  MISSED by every conv, dual and prep case; seen
                                                     prep 1 (lo 5.2 %)                                   only as stem form equality 6 (stem_u8.hip has
                                                                                                         its own split)
Mutants 7 and 10 are what the zero tolerance and the top-binade row are for: the hi plane of every convolution off by an ulp in
18 % of its outputs, or a lo plane that never rounds up, and no comparison with fp64 in test_pair_gpu.py fails.
"""
import pytest
import torch

import exact_conv as E
import exact_pair as P

pytestmark = pytest.mark.gpu


def _ops():
    from dirtorch_amd import ops
    return ops


def _h(t):
    """An fp32 CPU tensor of fp16 numbers (or None) -> its fp16 device plane."""
    return None if t is None else t.half().contiguous().cuda()


def _cpu(pair):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in pair)


CONV_ROWS = P.conv_rows()


@pytest.mark.parametrize('row', CONV_ROWS, ids=[r[0] + '-' + r[-1] for r in CONV_ROWS])
def test_conv_bn_act_pair_bitwise(row, monkeypatch):
    """Every operand form of one row: x a pair / a single plane (the _xw and _w kernels), the residual a pair / a single plane
    / absent, pair_out on / off; patch-kernel rows also behind DIRTORCH_AMD_NO_PAIR_PATCH, where the implicit-GEMM twin must
    give the same bits."""
    ops = _ops()
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
    o = P.pair_operands(row)
    d = P.PairOperands(*[_h(t) if t is not o.bias else t.cuda() for t in o])
    res_unit = P.row_resolution(row)
    BN = 128 if Cout % 128 == 0 else 64
    launches = 0
    for no_patch in ((False, True) if P.is_patch_row(row) else (False,)):
        if no_patch:
            monkeypatch.setenv('DIRTORCH_AMD_NO_PAIR_PATCH', '1')
        for x_pair in (True, False):
            for planes in ((2, 1) if use_res else (0,)):
                hi, lo, v = P.pair_reference(o, row, x_pair, planes)
                x = (d.x_hi, d.x_lo) if x_pair else d.x_hi
                res = None if planes == 0 else (d.res_hi, d.res_lo) if planes == 2 else d.res_hi
                for pair_out in (True, False):
                    y = ops.conv_bn_act_pair(x, (d.w_hi, d.w_lo), d.bias, res, stride=stride, pad=pad, relu=relu, pair_out=pair_out)
                    assert (y[1] is not None) == pair_out
                    what = '%s x %s, residual planes %d, pair_out %d%s' % (tag, 'pair' if x_pair else 'single', planes, pair_out,
                                                                           ', implicit GEMM' if no_patch else '')
                    P.mismatch_pair(_cpu(y), (hi, lo), what, 128, BN, v, res_unit)
                    launches += 1
    assert launches == (2 if P.is_patch_row(row) else 1) * 2 * (2 if use_res else 1) * 2


@pytest.mark.parametrize('shape', P.DUAL_SHAPES, ids=['%dx%dx%d-%d-%d' % s for s in P.DUAL_SHAPES])
def test_conv_pair_dual_bitwise_and_equal_to_the_two_launches(shape):
    """relu([w3 | wds] . [t2 ; x] + b3 + bds) in one launch against fp64 - and against downsample -> pair, conv3 + that pair as
    the residual: the downsample's output is a value its pair holds exactly (bit_budget 'pair_dual'), so the two paths form the
    same fp32 number and the same planes."""
    ops = _ops()
    B, H, W, C, Cout = shape
    o = P.dual_operands(shape)
    hi, lo, v = P.dual_reference(o)
    unit = P.row_resolution(P.dual_row(shape))
    tp, xp, wp = (_h(o.t_hi), _h(o.t_lo)), (_h(o.x_hi), _h(o.x_lo)), (_h(o.w_hi), _h(o.w_lo))
    for pair_out in (True, False):
        y = ops.conv_pair_dual(tp, xp, wp, (o.b3 + o.bd).cuda(), pair_out=pair_out)
        P.mismatch_pair(_cpu(y), (hi, lo), 'conv_pair_dual %r pair_out %d' % (shape, pair_out), 128, 128, v, unit)
    w3p = tuple(_h(t[:, :C].reshape(Cout, 1, 1, C)) for t in (o.w_hi, o.w_lo))
    wdp = tuple(_h(t[:, C:].reshape(Cout, 1, 1, C)) for t in (o.w_hi, o.w_lo))
    dsp = ops.conv_bn_act_pair(xp, wdp, o.bd.cuda(), None, relu=False)
    wd = lambda t: t[:, C:].reshape(Cout, 1, 1, C)      # noqa: E731
    dv = P.as_fp32(P.pair_value(o.x_hi, o.x_lo, wd(o.w_hi), wd(o.w_lo), o.bd, relu=False), 'downsample')
    P.mismatch_pair(_cpu(dsp), P.split_value(dv), 'the downsample launch %r' % (shape,), 128, 128, dv, 2.0 ** -7)
    two = ops.conv_bn_act_pair(tp, w3p, o.b3.cuda(), dsp, relu=True)
    P.mismatch_pair(_cpu(two), (hi, lo), 'downsample + conv3 in two launches %r' % (shape,), 128, 128, v, unit)


SEAM_CASES = [(s, r) for s in P.SEAM_WP_SHAPES for r in (True, False)]


@pytest.mark.parametrize('shape,relu3', SEAM_CASES, ids=['%dx%dx%d-P2_%d-w1%s-%s' % (s[:4] + ('pair' if s[4] else 'single', 'relu' if r else 'norelu'))
                                                         for s, r in SEAM_CASES])
def test_seam_with_paired_weights_bitwise(shape, relu3):
    """conv_c3c1_wpair: y = RNE(act3((w3_hi + w3_lo) . t2 + b3 + res)), t1 = RNE(relu((w1_hi + w1_lo) . RNE(y) + b1)), P2 = 64 and
    128, w1 a pair and (hi, None)."""
    ops = _ops()
    o = P.seam_wp_operands(shape, seed=E.zlib.crc32(repr((shape, False)).encode()))
    want_y, want_t1, vy, vt = P.seam_wp_reference(o, relu3)
    y, t1 = ops.conv_c3c1_wpair(_h(o.t2), (_h(o.w3_hi), _h(o.w3_lo)), o.b3.cuda(), _h(o.res), (_h(o.w1_hi), _h(o.w1_lo)), o.b1.cuda(),
                                relu3=relu3)
    torch.cuda.synchronize()
    what = 'conv_c3c1_wpair %r relu3 %d' % (shape, relu3)
    P.report_mismatch(y.cpu(), want_y, what + ': block output y', 64, 256, vy, 0.5)
    P.report_mismatch(t1.cpu(), want_t1, what + ': next conv1 t1', 64, shape[3], vt, 2.0 ** -7)


DS_CASES = [(s, f) for s in P.SEAM_DS_SHAPES for f in ('roles_split', 'one_role')]


@pytest.mark.parametrize('bhw,form', DS_CASES, ids=['%dx%dx%d-%s' % (s + (f,)) for s, f in DS_CASES])
def test_downsample_seam_with_paired_weights_bitwise(bhw, form, monkeypatch):
    """conv_c3c1_ds_wpair in conv_c3c1lc.hip's roles-split kernel and in conv_c3c1.hip's DS form (DIRTORCH_AMD_NO_C3C1LC): (w_hi +
    w_lo) . t2 + (wd_hi + wd_lo) . x_hi + wd_hi . x_lo + b; one, two and three tiles per workgroup, a ragged last tile."""
    if form == 'one_role':
        monkeypatch.setenv('DIRTORCH_AMD_NO_C3C1LC', '1')
    ops = _ops()
    shape = bhw + (64, True)
    o = P.seam_wp_operands(shape, ds=True, seed=E.zlib.crc32(repr((shape, True)).encode()))
    want_y, want_t1, vy, vt = P.seam_wp_reference(o)
    y, t1 = ops.conv_c3c1_ds_wpair(_h(o.t2), (_h(o.x_hi), _h(o.x_lo)), (_h(o.w3_hi), _h(o.w3_lo)), o.b3.cuda(),
                                   (_h(o.w1_hi), _h(o.w1_lo)), o.b1.cuda())
    torch.cuda.synchronize()
    what = 'conv_c3c1_ds_wpair %r %s' % (bhw, form)
    P.report_mismatch(y.cpu(), want_y, what + ': block output y', 64, 256, vy, 1.0)
    P.report_mismatch(t1.cpu(), want_t1, what + ': next conv1 t1', 64, 64, vt, 2.0 ** -7)


STEM_FORMS = {'default': None, 'one_tile_per_workgroup': 'DIRTORCH_AMD_STEM_V1', 'persistent_lds_tile': 'DIRTORCH_AMD_STEM_PAIR_OLD'}
STEM_CASES = [(s, f) for s in P.STEM_SIZES for f in STEM_FORMS]


@pytest.mark.parametrize('bhw,form', STEM_CASES, ids=['%dx%dx%d-%s' % (s + (f,)) for s, f in STEM_CASES])
def test_stem_pool_pair_bitwise(bhw, form, monkeypatch):
    """A lattice image pair (space-to-depth planes built on the CPU) and a lattice 7 x 7 filter through pack_stem_weight +
    split_pair: split(maxpool(relu(conv + bias))) in each of the three kernels, each against the reference."""
    if STEM_FORMS[form]:
        monkeypatch.setenv(STEM_FORMS[form], '1')
    ops = _ops()
    B, H, W = bhw
    o = P.stem_operands(bhw)
    hi, lo, v = P.stem_reference(o)
    wp = ops.split_pair(ops.pack_stem_weight(o.w.cuda(), torch.float32))
    want_w = tuple(ops.pack_stem_weight(t, torch.float16) for t in (o.w_hi, o.w_lo))
    assert torch.equal(wp[0].cpu(), want_w[0]) and torch.equal(wp[1].cpu(), want_w[1])      # the filter pair IS the lattice pair
    s2d = (_h(P.s2d(o.x_hi)), _h(P.s2d(o.x_lo)))
    y = ops.stem_pool_pair(s2d, wp, o.bias.cuda(), E.out_hw(H, W, 7, 2, 3))
    P.mismatch_pair(_cpu(y), (hi, lo), 'stem_pool_pair %dx%dx%d %s' % (B, H, W, form), 15, 64, v, P.row_resolution(P.stem_row(bhw)))


def test_prep_input_pair_f32_feed_is_split_pair_bitwise():
    """The fp32 feed normalises nothing: both planes are the CPU split of the same numbers - arbitrary fp32 values, not lattice
    ones: ordinary pixels, values whose lo is an fp16 subnormal, values whose hi is one, zeros, values at and beyond fp16's
    half-ulp ties; odd H and W, so the zero-filled space-to-depth border is compared too."""
    ops = _ops()
    g = torch.Generator().manual_seed(41)
    B, H, W = 2, 37, 51
    x = torch.randn(B, 3, H, W, generator=g) * 1.2
    x[:, :, 5:9] *= 2.0 ** -7                       # |x| ~ 1e-2: lo ~ 5e-6, a subnormal
    x[:, :, 9:12] *= 2.0 ** -16                     # hi itself a subnormal
    x[:, :, 12:14] = 0
    x[:, :, 14:16] = (torch.randint(1024, 2048, (B, 3, 2, W), generator=g).float() + 0.5) * 2.0 ** -10      # exact ties of hi
    x[:, :, 16:18] = torch.randint(-3, 4, (B, 3, 2, W), generator=g).float()                                  # lo == 0
    hi, lo = _cpu(ops.prep_input_pair(x.cuda()))
    want = ops.split_pair(P.s2d(x))
    sub = lambda t: float(((t != 0) & (t.float().abs() < E.FP16_MIN_NORMAL)).float().mean())      # noqa: E731
    assert sub(want[1]) > 0.05 and sub(want[0]) > 0.02 and float((want[1] == 0).float().mean()) > 0.25
    P.mismatch_pair((hi, lo), want, 'prep_input_pair fp32 feed %dx%dx%d' % (B, H, W), 64, 16)


U8_FORMS = {'default': None, 'prep': 'DIRTORCH_AMD_STEM_U8_PREP', 'one_workgroup_per_cu': 'DIRTORCH_AMD_STEM_U8_WG8'}
U8_CASES = [(s, f) for s in P.U8_SIZES for f in U8_FORMS]


@pytest.mark.parametrize('bhw,form', U8_CASES, ids=['%dx%dx%d-%s' % (s + (f,)) for s, f in U8_CASES])
def test_stem_pool_u8_bitwise(bhw, form, monkeypatch):
    """stem_pool_u8 against the reference's own definition (ToTensor, Normalize, conv, BN, ReLU, max-pool) in fp64, on operands
    for which the host's fold (filter pair, bias, border table) is exact (exact_pair.u8_fold asserts each step): the raw form
    (even widths, default), the prep form (odd widths, DIRTORCH_AMD_STEM_U8_PREP), the one-workgroup form, segments of the
    library's choice, of one and of two tiles."""
    if U8_FORMS[form]:
        monkeypatch.setenv(U8_FORMS[form], '1')
    ops = _ops()
    o = P.u8_operands(bhw)
    P.u8_fold(o)
    hi, lo, v = P.u8_reference(o)
    for seg_tiles in ((0, 1) if form == 'one_workgroup_per_cu' else (0, 1, 2)):      # (the forms and segment lengths test_stem_u8_gpu.py runs)
        y = ops.stem_pool_u8(o.img.cuda(), o.w, o.scale, o.bias, P.U8_MEAN, P.U8_STD, seg_tiles=seg_tiles)
        P.mismatch_pair(_cpu(y), (hi, lo), 'stem_pool_u8 %dx%dx%d %s seg_tiles %d' % (bhw + (form, seg_tiles)), 15, 64, v, 2.0 ** -15)

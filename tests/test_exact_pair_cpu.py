"""The conditions on the INPUTS of the bit-exact pair tests (tests/exact_pair.py), met by the CPU reference alone.

For every row tests/test_exact_pair_gpu.py uses:
  * bit_budget holds: at most 24 significant bits at every add, magnitudes under 65 504, every input plane an fp16 number;
  * the fp32 CPU evaluation of the three-product sum equals the fp64 one bit for bit;
  * rows with a ReLU: 30-70 % of the outputs are positive;
  * at least 30 % of the positive outputs cannot be held by hi alone, and at least 30 % have a non-zero lo: the second plane
    is exercised, not carried along;
  * every product matters: dropping w_hi.x_lo or w_lo.x_hi, or adding the w_lo.x_lo no kernel forms, changes at least 30 % of
    the outputs;
  * the top-binade row: at least 10 % of the outputs have hi + lo != v (lo itself rounds); the scaled row: at least 50 % of the
    non-zero outputs have a subnormal lo;
  * the seams: 30-70 % of t1 positive, at least 30 % of the positive t1 inexact in fp16 and at least 2 % exact ties
    (test_exact_lattice_cpu._check_stats' thresholds, in the one format these kernels exist in), y on fp16's grid.
A row that misses one is a badly chosen row, to be replaced.  Each test prints the bits used and the shares it measured.
"""
import pytest
import torch

import exact_conv as E
import exact_pair as P


def _pct(*shares):
    return ' / '.join('%.1f' % (100 * s) for s in shares)


def _conv_case(row):
    """One row: fp32 == fp64, the shares of its outputs, the weight of every product.  Returns the printed line."""
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
    bits = [p[3] for p in P.bit_budget(row)]
    o = P.pair_operands(row)
    args = (o.x_hi, o.x_lo, o.w_hi, o.w_lo, o.bias, o.res_hi, o.res_lo, stride, pad, relu)
    v64 = P.pair_value(*args)
    v32 = P.pair_value(*args, precision=torch.float32)
    assert torch.equal(v32.double(), v64), '%s: the fp32 and fp64 CPU sums differ on lattice operands' % tag
    hi, lo = P.split_value(v32)
    positive, hi_inexact, lo_nonzero, lo_rounds, lo_sub, hi_sub = P.pair_stats(v32, hi, lo)
    changed = {}
    for name, products in (('w_hi.x_lo dropped', ('hh', 'lh')), ('w_lo.x_hi dropped', ('hh', 'hl')),
                           ('w_lo.x_lo added', ('hh', 'hl', 'lh', 'll'))):
        changed[name] = float((P.pair_value(*args, products=products) != v64).float().mean())
    line = ('%-26s bits %s | positive %s %%, of those: hi inexact %s %%, lo != 0 %s %% | hi + lo != v %s %%, lo / hi subnormal %s %% '
            '| changed by: %s' % (tag, bits, _pct(positive), _pct(hi_inexact), _pct(lo_nonzero), _pct(lo_rounds),
                                  _pct(lo_sub, hi_sub), ', '.join('%s %s %%' % (n, _pct(c)) for n, c in changed.items())))
    if relu:
        assert 0.30 <= positive <= 0.70, line
    assert hi_inexact >= 0.30 and lo_nonzero >= 0.30, line
    assert all(c >= 0.30 for c in changed.values()), line
    if kind == 'top':
        assert lo_rounds >= 0.10, line
        assert float(v32.abs().min()) > 64 and float(v32.abs().max()) < 256, line
    if kind == 'scaled':
        assert lo_sub >= 0.50, line
        assert float(o.w_lo.abs().max()) < E.FP16_MIN_NORMAL, line
    return line


@pytest.mark.parametrize('row', P.conv_rows(), ids=[r[0] + '-' + r[-1] for r in P.conv_rows()])
def test_conv_rows_are_exact_and_exercise_both_planes(row):
    print('\n' + _conv_case(row))
    # the other operand forms of the same row: a single-plane x, fewer residual planes - subsets of the same terms
    for x_pair in (True, False):
        for planes in ((2, 1) if row[9] else (0,)):
            P.pair_reference(P.pair_operands(row), row, x_pair, planes)      # (asserts the fp64 value is an fp32 number)


@pytest.mark.parametrize('shape', P.DUAL_SHAPES, ids=['%dx%dx%d-%d-%d' % s for s in P.DUAL_SHAPES])
def test_dual_rows_and_their_two_launch_leg(shape):
    """conv_pair_dual's row as the paired convolution of K = 2 C, and the intermediate of the two launches it replaces: the
    downsample's output is a value its (hi, lo) pair holds exactly, so both paths form the same fp32 number."""
    bits = [p[3] for p in P.bit_budget(shape, 'pair_dual')]
    o = P.dual_operands(shape)
    B, H, W, C, Cout = shape
    hi, lo, v = P.dual_reference(o)
    wd = lambda t: t[:, C:].reshape(Cout, 1, 1, C)      # noqa: E731
    ds = P.as_fp32(P.pair_value(o.x_hi, o.x_lo, wd(o.w_hi), wd(o.w_lo), o.bd, relu=False), 'downsample')
    dh, dl = P.split_value(ds)
    assert torch.equal(dh.double() + dl.double(), ds.double()), 'the downsample pair does not hold its value'
    w3 = lambda t: t[:, :C].reshape(Cout, 1, 1, C)      # noqa: E731
    two = P.as_fp32(P.pair_value(o.t_hi, o.t_lo, w3(o.w_hi), w3(o.w_lo), o.b3, dh.float(), dl.float()), 'two launches')
    assert torch.equal(two, v)
    positive, hi_inexact, lo_nonzero = P.pair_stats(v, hi, lo)[:3]
    print('\n%s bits %s | positive %s %%, hi inexact %s %%, lo != 0 %s %%' % (shape, bits, _pct(positive), _pct(hi_inexact), _pct(lo_nonzero)))
    assert 0.30 <= positive <= 0.70 and hi_inexact >= 0.30 and lo_nonzero >= 0.30


def _seam_stats(vt, what):
    positive, inexact, ties = E.rounding_stats(vt, torch.float16)
    line = '%s: t1 positive %s %%, of those inexact in fp16 %s %%, exact ties %s %%' % (what, _pct(positive), _pct(inexact), _pct(ties))
    assert 0.30 <= positive <= 0.70 and inexact >= 0.30 and ties >= 0.02, line
    return line


@pytest.mark.parametrize('relu3', [True, False])
def test_seam_rows_chain_is_exact_and_rounding_is_exercised(relu3):
    for ds, shapes in ((False, P.SEAM_WP_SHAPES), (True, [s + (64, True) for s in P.SEAM_DS_SHAPES])):
        for shape in shapes:
            form = 'seam_ds_wp' if ds else 'seam_wp'
            bits = [p[3] for p in P.bit_budget(shape, form)]
            o = P.seam_wp_operands(shape, ds=ds, seed=E.zlib.crc32(repr((shape, ds)).encode()))
            y, t1, vy, vt = P.seam_wp_reference(o, relu3)      # (asserts both fp64 values are fp32 numbers)
            assert torch.equal(y.float(), vy), 'y left fp16\'s grid'
            # the lo planes matter: conv3's and conv1's
            y0 = P.seam_wp_reference(o._replace(w3_lo=torch.zeros_like(o.w3_lo)), relu3)[0]
            lo3 = float((y0 != y).float().mean())
            lo1 = 1.0
            if o.w1_lo is not None:
                lo1 = float((P.seam_wp_reference(o._replace(w1_lo=None), relu3)[1] != t1).float().mean())
            assert lo3 >= 0.30 and lo1 >= 0.30, (shape, lo3, lo1)
            print('\n' + _seam_stats(vt, '%s %r relu3 %d bits %s, changed without w3_lo %s %%, without w1_lo %s %%'
                                     % (form, shape, relu3, bits, _pct(lo3), _pct(lo1))))


@pytest.mark.parametrize('bhw', P.STEM_SIZES, ids=['%dx%dx%d' % s for s in P.STEM_SIZES])
def test_stem_rows(bhw):
    """The stem's row before the pool (all of _conv_case's conditions on the 7 x 7 convolution), the filter's split, and the
    pooled reference: the split commutes with the max."""
    row = P.stem_row(bhw)
    o = P.stem_operands(bhw)
    nhwc = lambda t: t.permute(0, 2, 3, 1)      # noqa: E731
    bits = [p[3] for p in P.bit_budget(row)]
    args = (nhwc(o.x_hi), nhwc(o.x_lo), nhwc(o.w_hi), nhwc(o.w_lo), o.bias, None, None, 2, 3, True)
    v64 = P.pair_value(*args)
    v32 = P.pair_value(*args, precision=torch.float32)
    assert torch.equal(v32.double(), v64)
    ch, cl = P.split_value(v32)
    positive, hi_inexact, lo_nonzero = P.pair_stats(v32, ch, cl)[:3]
    changed = [float((P.pair_value(*args, products=pr) != v64).float().mean()) for pr in (('hh', 'lh'), ('hh', 'hl'), ('hh', 'hl', 'lh', 'll'))]
    hi, lo, v = P.stem_reference(o)
    pool = lambda t: torch.nn.functional.max_pool2d(t.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)      # noqa: E731
    assert torch.equal(hi.float(), pool(ch))      # hi of the max == max of the his (RNE is monotone)
    ph, pl = P.pair_stats(v, hi, lo)[1:3]
    print('\n%s bits %s | conv: positive %s %%, hi inexact %s %%, lo != 0 %s %%, changed by a dropped / added product %s %% | pooled: '
          'hi inexact %s %%, lo != 0 %s %%' % (row[0], bits, _pct(positive), _pct(hi_inexact), _pct(lo_nonzero), _pct(*changed), _pct(ph), _pct(pl)))
    assert 0.30 <= positive <= 0.70 and hi_inexact >= 0.30 and lo_nonzero >= 0.30 and min(changed) >= 0.30
    assert ph >= 0.30 and pl >= 0.30


def test_bit_budget_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):      # K = 9 x 2 048: the products alone pass 65 504
        P.bit_budget(('too_long', 1, 8, 8, 2048, 64, 3, 1, 1, False, True, 'std'))
    with pytest.raises(AssertionError):      # a residual on the scaled row: its planes are not scaled
        P.bit_budget(('scaled_res', 1, 8, 8, 64, 64, 1, 1, 0, True, True, 'scaled'))
    with pytest.raises(AssertionError):      # the two-launch leg at K = 2 x 8 192: the downsample's output no longer fits a pair
        P.bit_budget((1, 8, 8, 8192, 256), 'pair_dual')
    assert P.bit_budget(E.ANCHOR_ROW, 'conv') == E.bit_budget(E.ANCHOR_ROW)      # every other form is exact_conv's


@pytest.mark.parametrize('bhw', P.U8_SIZES, ids=['%dx%dx%d' % s for s in P.U8_SIZES])
def test_u8_stem_fold_and_reference_are_exact(bhw):
    """The uint8 stem: every step of the host's fold is exact on these operands (u8_fold asserts each), the reference's literal
    chain agrees with its exact rearrangement, and the pooled outputs exercise both planes."""
    bits = [p[3] for p in P.u8_budget()]
    o = P.u8_operands(bhw)
    wp, b2 = P.u8_fold(o)
    hi, lo, v = P.u8_reference(o)
    positive, hi_inexact, lo_nonzero = P.pair_stats(v, hi, lo)[:3]
    print('\nstem_u8 %r bits %s | positive %s %%, of those: hi inexact %s %%, lo != 0 %s %%' % (bhw, bits, _pct(positive), _pct(hi_inexact), _pct(lo_nonzero)))
    assert 0.30 <= positive <= 0.70 and hi_inexact >= 0.30 and lo_nonzero >= 0.30
    assert float(torch.tensor(P.U8_MEAN).abs().min()) > 0      # a non-zero mean: the border-class table is in play

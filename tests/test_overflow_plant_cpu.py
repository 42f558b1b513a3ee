"""The preconditions of tests/overflow_plant.py, on the CPU: for every plant test_overflow_word_gpu.py makes, the fp32 / fp64
reference of the same rounded operands is non-finite in fp16 exactly where the plant intends - and finite everywhere in
bf16 - so that a change to a shape table or to the random operands cannot quietly void the GPU test.  No library calls."""
import pytest
import torch

import overflow_plant as P
from test_ops_gpu import CONV_SHAPES, DUAL_SHAPES, SEAM_SHAPES, SPLITK_SHAPES

ROWS = [(s[0], s) for s in CONV_SHAPES if P.small(s)] + [('splitk/' + s[0], s) for s in SPLITK_SHAPES if P.small(s)]


def test_the_shape_tables_still_hold_the_rows_the_gpu_test_names():
    assert len(ROWS) == 28 and all(P.small(s) for s in SPLITK_SHAPES)
    big = [s[0] for s in CONV_SHAPES if not P.small(s)]
    assert big == ['3x3_s2_persistent']       # the row whose persistent workgroups walk several tiles: device checker there
    assert (4, 80, 80) in SEAM_SHAPES and (1, 5, 7) in SEAM_SHAPES and (2, 37, 29) in SEAM_SHAPES


@pytest.mark.parametrize('name,shape', ROWS, ids=[r[0] for r in ROWS])
def test_single_plant_is_a_singleton_in_fp16_and_nothing_in_bf16(name, shape):
    """Five positions x both signs on every small row (280 plants in all): {(m, n)} for +1024 or without a ReLU, nothing for
    -1024 under a ReLU; the clean operands overflow nowhere."""
    assert P.conv_expected(name, 'fp16', ()) == frozenset()
    assert float(P.conv_output(shape, P.conv_case(name, 'fp16')).abs().max()) < 16
    plants = P.conv_plants(shape, every_sign=True)
    assert len(plants) == 10
    for m, n, sign, edits, intended in plants:
        assert P.conv_expected(name, 'fp16', edits) == intended, (name, m, n, sign)
    for m, n, sign, edits, intended in P.conv_plants(shape)[:2]:
        assert P.conv_expected(name, 'bf16', edits) == frozenset(), (name, m, n, sign)


@pytest.mark.parametrize('name,shape', ROWS, ids=[r[0] for r in ROWS])
def test_cancelling_pair_is_finite_everywhere(name, shape):
    for m, n in P.conv_cancel_positions(shape):
        edits = tuple(P.conv_cancelling(shape, m, n))
        assert P.conv_expected(name, 'fp16', edits) == frozenset(), (name, m, n)
        y = P.conv_output(shape, P.planted(P.conv_case(name, 'fp16'), edits))
        assert float(y.abs().max()) < 8192      # ... and nowhere near the edge: 1024 |x| and 256 |w| beside the clean sums


def test_boundary_case_rounds_to_65504_and_to_inf():
    shape = CONV_SHAPES[0]
    M, Cout = P.geom(shape)[12], shape[5]
    m, n = P.positions(M, Cout)[4]
    for bias_n, want in ((15.0, 65504.0), (16.0, float('inf'))):
        c = P.conv_boundary(shape, m, n, bias_n)
        y32 = P.conv_reference(c['x'], c['w'], c['bias'], c['res'], shape[7], shape[8], False).reshape(M, Cout)
        assert float(y32[m, n]) == 65504.0 + bias_n       # exact in fp32
        y16 = y32.half()
        assert float(y16[m, n]) == want
        y16[m, n] = bias_n
        assert bool((y16[:, n] == bias_n).all())      # the bias alone in the rest of channel n, zero in every other
        y16[:, n] = 0
        assert float(y16.abs().max()) == 0.0


SEAM_SMALL = [s for s in SEAM_SHAPES if s[0] * s[1] * s[2] < 5000]


@pytest.mark.parametrize('relu3', [True, False])
@pytest.mark.parametrize('P1,P2', P.SEAM_PLANES)
@pytest.mark.parametrize('B,H,W', SEAM_SMALL)
def test_seam_plants(B, H, W, P1, P2, relu3):
    case = P.seam_case(B, H, W, P1, P2, 'fp16')
    M = B * H * W
    assert P.seam_expected(case, 'fp16', relu3) == (frozenset(), frozenset())
    for m, n in ((0, 0), (1, 4 * P1 - 1), (M - 1, 2 * P1 + 1)):
        ey, et = P.seam_expected(P.planted(case, P.seam_plant_y(case, m, n)), 'fp16', relu3)
        assert ey == frozenset([(m, n)])
        assert et and all(mm == m for mm, _ in et)      # conv1 reads the stored inf: row m of t1, and only row m
        # pixel 0 is on an even row and column (stored at a stage exit), pixel 1 = (0, 0, 1) is not, the last one is here
        assert P.seam_expected(P.planted(case, P.seam_plant_y(case, m, n)), 'fp16', relu3, keep_stride=2) == (
            frozenset() if m == 1 else ey, et)
    ey, et = P.seam_expected(P.planted(case, P.seam_plant_y(case, 0, 0, -1)), 'fp16', relu3)
    assert (ey, et) == ((frozenset(), frozenset()) if relu3 else (frozenset([(0, 0)]), et)) and (relu3 or et)
    for m, n2 in P.positions(M, P2)[1:3]:
        ey, et = P.seam_expected(P.planted(case, P.seam_plant_t1(case, m, n2)), 'fp16', relu3)
        assert (ey, et) == (frozenset(), frozenset([(m, n2)]))
    bf = P.seam_case(B, H, W, P1, P2, 'bf16')
    assert P.seam_expected(P.planted(bf, P.seam_plant_y(bf, M - 1, 4 * P1 - 1)), 'bf16', relu3) == (frozenset(), frozenset())


@pytest.mark.parametrize('form', ['ds', 'wp', 'ds_wp'])
def test_seam_plants_of_the_downsample_and_paired_forms(form):
    B, H, W = 2, 37, 29
    case = P.seam_case(B, H, W, 64, 64, 'fp16', form)
    M = B * H * W
    assert P.seam_expected(case, 'fp16', True) == (frozenset(), frozenset())
    ey, et = P.seam_expected(P.planted(case, P.seam_plant_y(case, M - 1, 255)), 'fp16', True)
    assert ey == frozenset([(M - 1, 255)]) and et and all(mm == M - 1 for mm, _ in et)
    ey, et = P.seam_expected(P.planted(case, P.seam_plant_t1(case, M - 1, 63)), 'fp16', True)
    assert (ey, et) == (frozenset(), frozenset([(M - 1, 63)]))


@pytest.mark.parametrize('shape', DUAL_SHAPES, ids=['%dx%dx%d-%d-%d-%d-s%d' % s for s in DUAL_SHAPES])
def test_two_source_plants(shape):
    B, OH, OW, Cin, Cout, Cin2, s2 = shape
    case = P.dual_case(*shape, 'fp16')
    assert P.dual_expected(case, s2, 'fp16', True) == frozenset()
    for i, (m, n) in enumerate(P.positions(B * OH * OW, Cout)):
        assert P.dual_expected(P.planted(case, P.dual_plant(case, s2, m, n, i % 2)), s2, 'fp16', True) == frozenset([(m, n)])
    assert P.dual_expected(P.planted(case, P.dual_plant(case, s2, 0, 0, 1, -1)), s2, 'fp16', True) == frozenset()
    assert P.dual_expected(P.planted(case, P.dual_cancelling(case, s2, B * OH * OW - 1, Cout - 1)), s2, 'fp16', True) == frozenset()


def test_paired_plants():
    from test_pair_gpu import GEOMS
    for g in GEOMS:
        B, H, W, Cin, Cout, k, stride, pad, with_res, relu = g
        M = B * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1)
        case = P.pair_case(g)
        assert P.pair_expected(g, case) == frozenset()
        for m, n in P.positions(M, Cout)[1::3]:
            assert P.pair_expected(g, P.planted(case, P.pair_plant(g, m, n))) == frozenset([(m, n)])
        assert P.pair_expected(g, P.planted(case, P.pair_plant(g, 0, 0, -1))) == (frozenset() if relu else frozenset([(0, 0)]))
    for s in P.PAIR_DUAL_SHAPES:
        case = P.pair_dual_case(*s)
        M = s[0] * s[1] * s[2]
        assert P.pair_dual_expected(case, True) == frozenset()
        for src in (0, 1):
            assert P.pair_dual_expected(P.planted(case, P.pair_dual_plant(case, M - 1, s[4] - 1, src)), True) == frozenset([(M - 1, s[4] - 1)])


@pytest.mark.parametrize('H,W', P.STEM_SIZES)
def test_stem_plants_spread_over_the_pool_windows(H, W):
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    case = P.stem_case(H, W)
    assert P.stem_expected(case, 'fp16') == frozenset() and P.stem_pair_expected(case) == frozenset()
    for b, oh, ow, n in ((0, 0, 0, 0), (1, OH - 1, OW - 1, 63), (1, 5, 4, 33), (0, 4, 5, 7)):
        got = P.stem_expected(P.planted(case, P.stem_plant(b, oh, ow, n)), 'fp16')
        want = P.pool_windows(b, oh, ow, n, OH, OW)      # 2 ph - 1 <= oh <= 2 ph + 1, and so for the columns
        assert got == want and 1 <= len(want) <= 4
        assert P.stem_pair_expected(P.planted(case, P.stem_plant(b, oh, ow, n))) == want
        assert P.stem_expected(P.planted(case, P.stem_plant(b, oh, ow, n)), 'bf16') == frozenset()
    assert P.stem_expected(P.planted(case, P.stem_plant(0, 3, 3, 5, sign=-1)), 'fp16') == frozenset()      # ReLU first


@pytest.mark.parametrize('H,W', [(40, 52), (41, 53)])
def test_uint8_stem_plant(H, W):
    """20 x 26 (21 x 27) conv pixels, 10 x 13 (11 x 14) pooled ones"""
    PH, PW = ((H - 1) // 2) // 2 + 1, ((W - 1) // 2) // 2 + 1
    u8 = P.stem_u8_case(2, H, W)
    assert P.stem_u8_expected(u8) == frozenset()
    got = P.stem_u8_expected(P.planted(u8, P.stem_u8_plant(u8, 1, 5, 4, 33)))
    assert got == frozenset(((PH + ph) * PW + 2, 33) for ph in (2, 3)) == P.pool_windows(1, 5, 4, 33, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    assert P.stem_u8_expected(P.planted(u8, P.stem_u8_plant(u8, 1, 5, 4, 33)), torch.float32) == got


@pytest.mark.parametrize('shape', P.UPSAMPLE_SHAPES)
def test_upsample_add_plants(shape):
    B, H, W, h, w, C = shape
    case = P.upsample_case(*shape, 'fp16')
    assert P.upsample_expected(case, 'fp16') == frozenset()
    for m, n in P.positions(B * H * W, C):
        assert P.upsample_expected(P.planted(case, P.upsample_plant(case, m, n)), 'fp16') == frozenset([(m, n)])
    bf = P.upsample_case(*shape, 'bf16')
    assert P.upsample_expected(P.planted(bf, P.upsample_plant(bf, 0, 0)), 'bf16') == frozenset()

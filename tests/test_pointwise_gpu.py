"""The pointwise kernels at their loop edges (csrc/pointwise.hip and the fp32 twins of csrc/conv_f32.hip), through ops.* only,
against the references of tests/pointwise_ref.py (pinned on the CPU by tests/test_pointwise_ref_cpu.py).

Exact wherever exactness can be arranged:
  max, max-pool, upsample_add, the layout of prep_input    the reference's own bits
  avg / multiscale mean of integers                        the fp32 sum is exact in any order, one division is left: <= 1 fp32 ulp
                                                           of the fp64 quotient (0 where the device division rounds correctly)
  GeM p = 3 of integers in [-3, 7]                         exact sum of cubes, then a division (2^-24), the fp32 rounding of 1/p
                                                           (ln(343)/3 * 2^-25 = 6e-8) and one powf: 1e-6 relative to fp64, 8 ulps
  prep_input from uint8                                    ((u / 255) - mean) / std in numpy float32, rounded to nearest even
and the project's own tolerances where the arithmetic is transcendental or the inputs random (GeM p = 2.7 and centre bias:
rtol 2e-5, atol 1e-6 of test_ops_gpu.test_global_pool; L2 rows: rtol 2e-6, atol 1e-7; multiscale gem: rtol 2e-5, atol 1e-6), every
one against fp64.  Each bounded case prints its largest error.
"""
import numpy as np
import pytest
import torch

import pointwise_ref as R

pytestmark = pytest.mark.gpu

KINDS = ['bf16', 'fp16', 'f32']
DT = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'f32': torch.float32}


def _ops():
    from dirtorch_amd import ops
    return ops


def _rounded(x, kind):
    """(device tensor in the kind's storage type, the same values as fp32 numpy: what the kernel reads)"""
    t = torch.tensor(x).to(DT[kind])
    return t.cuda(), t.float().numpy()


def _global_pool(xd, kind, mode, p=3.0, cb=0.0):
    ops = _ops()
    fn = ops.global_pool_f32 if kind == 'f32' else ops.global_pool
    return fn(xd, mode, p, 1e-6, cb).cpu().numpy()


def _global_cases(hw):
    H, W = hw
    return [(B, H, W, C) for C in R.global_channels(H, W) for B in R.GLOBAL_BATCHES]


# ---- global pooling ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.GLOBAL_SIZES)
def test_global_pool_max_is_exact(hw, kind):
    for shape in _global_cases(hw):
        xd, xr = _rounded(R.signed_map(*shape), kind)
        want = R.global_pool_ref(xr, 'max').astype(np.float32)
        assert (want[0, :64] < 0).all()
        got = _global_pool(xd, kind, 'max')
        assert np.array_equal(got, want), 'max %s %s: %d of %d differ' % (shape, kind, (got != want).sum(), got.size)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.GLOBAL_SIZES)
def test_global_pool_avg_of_integers_is_one_division(hw, kind):
    worst, inexact = 0.0, 0
    for shape in _global_cases(hw):
        x = R.int_map(*shape)
        xd, xr = _rounded(x, kind)
        assert np.array_equal(xr, x)
        got = _global_pool(xd, kind, 'avg')
        ulps = R.ulps_f32(got, R.global_pool_ref(x, 'avg'))
        worst = max(worst, float(ulps.max()))
        inexact += int((got != x.sum(axis=(1, 2), dtype=np.float32) / np.float32(shape[1] * shape[2])).sum())
        assert ulps.max() <= 1.0, 'avg %s %s: %.3f ulps at (b, c) = %s' % (shape, kind, ulps.max(),
                                                                          np.unravel_index(ulps.argmax(), ulps.shape))
    print('\n[pointwise] avg of integers %dx%d %s: worst %.3f fp32 ulps of the fp64 quotient, %d outputs not the correctly rounded one'
          % (hw[0], hw[1], kind, worst, inexact))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.GLOBAL_SIZES)
def test_global_pool_gem3_of_integers(hw, kind):
    """The largest error sits on the channels with nothing positive, whose result is the clamp: the fp32 rounding of 1/3
    (9.9e-9) acts on ln(1e-18) = -41.4 there, not on ln(343), and moves the result by 4.1e-7 - powf(1e-18f, 1.f / 3.f) is
    1e-6 (1 - 4.55e-7) on the host as well.  Both groups of channels are held to the one bound and printed apart."""
    worst, worst_clamp = 0.0, 0.0      # (worst: every other channel - at a few pixels some of those are clamps too)
    for shape in _global_cases(hw):
        x = R.int_map(*shape)
        xd, _ = _rounded(x, kind)
        ref = R.global_pool_ref(x, 'gem', 3.0)
        for c in R.nonpos_channels(shape[3]):      # nothing positive: (HW eps^3 / HW)^(1/3), the clamp itself
            np.testing.assert_allclose(ref[:, c], R.F32_EPS_GEM, rtol=1e-12)
        got = _global_pool(xd, kind, 'gem', 3.0)
        rel = np.abs(got.astype(np.float64) - ref) / ref
        clamp = list(R.nonpos_channels(shape[3]))
        worst_clamp = max(worst_clamp, float(rel[:, clamp].max()))
        worst = max(worst, float(np.delete(rel, clamp, axis=1).max()))
        assert rel.max() <= 1e-6, 'gem3 %s %s: %.3g relative at (b, c) = %s' % (shape, kind, rel.max(),
                                                                              np.unravel_index(rel.argmax(), rel.shape))
    print('\n[pointwise] gem p=3 of integers %dx%d %s: worst relative error %.3g, on the all-non-positive channels %.3g '
          '(bound 1e-6)' % (hw[0], hw[1], kind, worst, worst_clamp))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.GLOBAL_SIZES)
def test_global_pool_gem27_and_centre_bias(hw, kind):
    worst = 0.0
    for shape in _global_cases(hw):
        xd, xr = _rounded(R.rand_map(*shape), kind)
        plain = {}
        for mode, p, cb in [('gem', 2.7, 0.0), ('avg', 3.0, 0.0), ('gem', 2.7, 0.5), ('gem', 2.7, 1.5), ('avg', 3.0, 0.5),
                            ('avg', 3.0, 1.5)]:
            got = _global_pool(xd, kind, mode, p, cb)
            ref = R.global_pool_ref(xr, mode, p, cb=cb)
            worst = max(worst, R.max_excess(got, ref, 2e-5, 1e-6))
            np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6, err_msg='%s p=%s cb=%s %s %s' % (mode, p, cb, shape, kind))
            if cb == 0.0:
                plain[mode] = got
            elif 1 in hw:       # a single row or column samples the mask's zero border: the mask is exactly 1
                assert np.array_equal(got, plain[mode]), '%s cb=%s %s %s: the mask of a %dx%d map is not 1' % (
                    mode, cb, shape, kind, hw[0], hw[1])
    print('\n[pointwise] gem p=2.7 / avg, centre bias 0, 0.5, 1.5, %dx%d %s: worst |err| / (1e-6 + 2e-5 |ref|) = %.3g'
          % (hw[0], hw[1], kind, worst))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', [(3, 43), (32, 32)])
def test_global_pool_counts_every_pixel_once(hw, kind):
    """Image i of the batch holds 64 at pixel i and 0 elsewhere: its average is 64 / HW exactly, and a pixel that a lane row
    skips or reads twice is named by its position."""
    H, W = hw
    HW = H * W
    x = torch.zeros(HW, HW, 64, dtype=DT[kind], device='cuda')
    i = torch.arange(HW, device='cuda')
    x[i, i, :] = 64.0
    got = _global_pool(x.view(HW, H, W, 64), kind, 'avg')
    want = np.float32(64.0) / np.float32(HW)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, 'avg %dx%d %s: pixels %s give %s, not %r' % (H, W, kind, bad[:8], got[bad[:8], 0], want)


# ---- max-pool 3x3 stride 2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.MAXPOOL_SIZES)
def test_maxpool_is_exact(hw, kind):
    ops = _ops()
    H, W = hw
    chans = (4, 64) if kind == 'f32' else ((8, 64, 2048) if hw == (7, 12) else (8, 64))
    for C in chans:
        xd, xr = _rounded(R.maxpool_map(2, H, W, C), kind)
        want = R.maxpool_ref(xr)
        assert (want[1] < 0).all()
        got = (ops.maxpool_3x3s2_f32(xd) if kind == 'f32' else ops.maxpool_3x3s2(xd)).float().cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(got, want), 'maxpool %dx%dx%d %s: %d of %d differ' % (H, W, C, kind, (got != want).sum(), got.size)


# ---- prep_input -------------------------------------------------------------------------------------------------------
def _prep(img, kind, mean=None, std=None):
    ops = _ops()
    if kind == 'f32':
        return ops.prep_input_f32(img, mean, std).cpu()
    return ops.prep_input(img, DT[kind], mean, std).cpu()


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('hw', R.PREP_SIZES)
def test_prep_input_whole_tensor(hw, kind):
    H, W = hw
    for B in (1, 3):
        # fp32 NCHW feed: a permutation (and one rounding to a 16-bit type)
        img = R.f32_image(B, H, W)
        want = torch.tensor(R.space_to_depth_ref(img.transpose(0, 2, 3, 1))).to(DT[kind])
        got = _prep(torch.tensor(img).cuda(), kind)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got, want), 'prep f32 feed %dx%d B=%d %s' % (H, W, B, kind)
        # uint8 NHWC feed: ToTensor + Normalize fused in, in the reference's order of operations
        u8 = R.u8_image(B, H, W)
        want = torch.tensor(R.space_to_depth_ref(R.normalize_u8_f32(u8))).to(DT[kind])
        got = _prep(torch.tensor(u8).cuda(), kind, list(R.MEAN), list(R.STD))
        assert got.shape == want.shape and got.dtype == want.dtype
        # layout and zeros first (exact whatever the arithmetic): a zero of the reference is a zero of the kernel, and only those
        assert torch.equal(got == 0, want == 0), 'prep u8 feed %dx%d B=%d %s: zero pattern' % (H, W, B, kind)
        assert float(got[..., 12:].abs().max()) == 0.0
        diff = (got != want)
        assert not diff.any(), 'prep u8 feed %dx%d B=%d %s: %d of %d values differ from the fp32 computation, first at %s' % (
            H, W, B, kind, int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist())


# ---- upsample_add (fp32 twin) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.UPSAMPLE_SHAPES)
def test_upsample_add_f32_is_one_add(shape):
    x, low = R.upsample_inputs(shape)
    got = _ops().upsample_add_f32(torch.tensor(x).cuda(), torch.tensor(low).cuda()).cpu().numpy()
    want = R.upsample_add_ref(x, low)
    assert np.array_equal(got, want), 'upsample_add_f32 %s: %d of %d differ' % (shape, (got != want).sum(), got.size)


# ---- row L2 norm ------------------------------------------------------------------------------------------------------
def _l2(x, *eps):
    return _ops().l2norm_rows_(torch.tensor(x).cuda(), *eps).cpu().numpy()


@pytest.mark.parametrize('cols', R.L2_COLS)
def test_l2norm_rows(cols):
    worst = 0.0
    for rows in R.L2_ROWS:
        x = R.l2_rows(rows, cols)
        got, ref = _l2(x), R.l2norm_ref(x)
        worst = max(worst, R.max_excess(got, ref, 2e-6, 1e-7))
        np.testing.assert_allclose(got, ref, rtol=2e-6, atol=1e-7, err_msg='l2norm %dx%d' % (rows, cols))
        if cols in (64, 256):       # norm 8 or 16: every output is +-2^-3 or +-2^-4
            u = R.unit_sign_rows(rows, cols)
            assert np.array_equal(_l2(u), u / np.float32(np.sqrt(cols)))
    print('\n[pointwise] l2norm_rows cols=%d: worst |err| / (1e-7 + 2e-6 |ref|) = %.3g' % (cols, worst))


@pytest.mark.parametrize('cols', R.L2_COLS)
def test_l2norm_rows_zero_and_tiny_rows(cols):
    x = R.l2_rows(5, cols)
    x[1] = 0.0
    x[4] = 0.0
    x[2] = R.l2_rows(1, cols)[0] * np.float32(1e-14)      # norm ~1e-14 sqrt(cols) < eps = 1e-12, squares still normal fp32
    live = [0, 3]
    got = _l2(x)
    assert (got[1] == 0).all() and (got[4] == 0).all()      # 0 * (1 / eps)
    np.testing.assert_allclose(got[live], R.l2norm_ref(x)[live], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(got[2], x[2].astype(np.float64) / 1e-12, rtol=2e-6, atol=0)
    # eps = 0, the whiten_features contract: a zero row is 0 * inf = NaN throughout, as the reference's division by
    # np.linalg.norm gives, and no other row of the call notices
    nan = _l2(x, 0.0)
    assert np.isnan(nan[1]).all() and np.isnan(nan[4]).all()
    assert np.array_equal(nan[live], got[live])
    np.testing.assert_allclose(nan[2], R.l2norm_ref(x, 0.0)[2], rtol=2e-6, atol=1e-7)
    z = np.zeros((1, cols), np.float32)
    assert (_l2(z) == 0).all() and np.isnan(_l2(z, 0.0)).all()


# ---- multi-scale pooling ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', R.MULTISCALE_SHAPES)
def test_multiscale_mean_of_integers_is_one_division(shape):
    x = R.multiscale_int_input(*shape)
    got = _ops().multiscale_pool(torch.tensor(x).cuda(), 'mean').cpu().numpy()
    ulps = R.ulps_f32(got, R.multiscale_pool_ref(x, 'mean'))
    inexact = int((got != x.sum(axis=0, dtype=np.float32) / np.float32(shape[0])).sum())
    print('\n[pointwise] multiscale mean %s: worst %.3f fp32 ulps of the fp64 quotient, %d outputs not the correctly rounded one'
          % (shape, ulps.max(), inexact))
    assert ulps.max() <= 1.0


@pytest.mark.parametrize('p', [3.0, 2.5])
@pytest.mark.parametrize('shape', R.MULTISCALE_SHAPES)
def test_multiscale_gem(shape, p):
    x = R.multiscale_gem_input(*shape, p)
    got = _ops().multiscale_pool(torch.tensor(x).cuda(), 'gem', p).cpu().numpy()
    ref = R.multiscale_pool_ref(x, 'gem', p)
    print('\n[pointwise] multiscale gem p=%s %s: worst |err| / (1e-6 + 2e-5 |ref|) = %.3g' % (p, shape, R.max_excess(got, ref, 2e-5, 1e-6)))
    assert got.reshape(-1)[R.MS_ZERO_COL] == 0.0 and ref.reshape(-1)[R.MS_ZERO_COL] == 0.0      # sign(0) = 0, not the clamp
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-6)

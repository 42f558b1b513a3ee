"""What tests/test_pointwise_gpu.py stands on, checked without a GPU: the references of tests/pointwise_ref.py agree with the
CPU oracle and with torch's own functions on the very inputs the GPU tests use, the 'exact' inputs are exact in both 16-bit
formats with every partial sum below 2^24, and the new fp32 entry points refuse what their 16-bit counterparts refuse."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R


def _nchw(x):
    return torch.from_numpy(np.array(x)).permute(0, 3, 1, 2)


@pytest.mark.parametrize('hw', [(1, 1), (1, 31), (127, 1), (3, 43), (13, 20)])
def test_global_pool_ref_is_the_oracle(hw):
    import dir_oracle as O
    H, W = hw
    x = R.rand_map(3, H, W, 64)
    xt = _nchw(x)
    for p in (3.0, 2.7):
        ref = R.global_pool_ref(x, 'gem', p)
        np.testing.assert_allclose(O.gem_pool(xt, p).reshape(3, 64).numpy(), ref, rtol=2e-6, atol=0)
    np.testing.assert_allclose(F.adaptive_avg_pool2d(xt, 1).reshape(3, 64).numpy(), R.global_pool_ref(x, 'avg'), rtol=0, atol=2e-6)
    s = R.signed_map(3, H, W, 64)
    assert np.array_equal(F.adaptive_max_pool2d(_nchw(s), 1).reshape(3, 64).numpy(), R.global_pool_ref(s, 'max').astype(np.float32))
    assert (R.global_pool_ref(s, 'max')[0] < 0).all()
    for cb in (0.5, 1.5):
        masked = xt * O.center_bias_mask(cb, (H, W))
        np.testing.assert_allclose(O.gem_pool(masked, 2.7).reshape(3, 64).numpy(), R.global_pool_ref(x, 'gem', 2.7, cb=cb), rtol=2e-6, atol=0)
        np.testing.assert_allclose(F.adaptive_avg_pool2d(masked, 1).reshape(3, 64).numpy(), R.global_pool_ref(x, 'avg', cb=cb),
                                   rtol=0, atol=2e-6)


@pytest.mark.parametrize('hw', R.GLOBAL_SIZES + [(2, 2), (31, 1), (5, 4)])
def test_center_mask_ref_is_the_oracle_and_one_on_a_single_row_or_column(hw):
    import dir_oracle as O
    for cb in (0.5, 1.5):
        mask = O.center_bias_mask(cb, hw)[0, 0].numpy()
        np.testing.assert_allclose(mask, R.center_mask_ref(cb, *hw), rtol=0, atol=4e-7 * (1 + cb))
        if 1 in hw:
            assert (mask == 1.0).all() and (R.center_mask_ref(cb, *hw) == 1.0).all()
    # 2 x 2 samples the four zero corners of the 4x4 mask
    assert (O.center_bias_mask(1.5, (2, 2)).numpy() == 1.0).all() and (R.center_mask_ref(1.5, 2, 2) == 1.0).all()
    assert R.center_mask_ref(1.5, 4, 4)[1, 1] == 2.5 and R.center_mask_ref(1.5, 4, 4)[0, 1] == 1.0


@pytest.mark.parametrize('hw', R.MAXPOOL_SIZES)
def test_maxpool_ref_is_max_pool2d(hw):
    for C in (4, 8):
        x = R.maxpool_map(2, hw[0], hw[1], C)
        ref = F.max_pool2d(_nchw(x), 3, 2, 1).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(R.maxpool_ref(x), ref)
        assert (ref[1] < 0).all()
        for dt in (torch.bfloat16, torch.float16):      # the max of rounded values is the rounded max
            xr = torch.tensor(x).to(dt).float().numpy()
            assert np.array_equal(R.maxpool_ref(xr), torch.from_numpy(ref).to(dt).float().numpy())


@pytest.mark.parametrize('shape', R.UPSAMPLE_SHAPES)
def test_upsample_add_ref_is_interpolate_nearest(shape):
    B, H, W, h, w, C = shape
    x, low = R.upsample_inputs(shape)
    up = F.interpolate(_nchw(low), size=(H, W), mode='nearest').permute(0, 2, 3, 1)
    assert np.array_equal(R.upsample_add_ref(x, low), (torch.from_numpy(x) + up).numpy())
    if (H, W) == (h, w):
        assert np.array_equal(R.upsample_add_ref(x, low), x + low)


@pytest.mark.parametrize('hw', R.PREP_SIZES)
def test_prep_refs(hw):
    H, W = hw
    for B in (1, 3):
        u8 = R.u8_image(B, H, W)
        assert u8.dtype == np.uint8 and u8.shape == (B, H, W, 3)
        if H * W >= 256:
            for b in range(B):
                for c in range(3):
                    assert len(np.unique(u8[b, :, :, c])) == 256
        f32 = R.normalize_u8_f32(u8)
        assert f32.dtype == np.float32
        # ToTensor + Normalize as torch computes them on the CPU; fp32 against fp64: three roundings of values below 3
        t = (torch.from_numpy(u8).float() / 255.0 - torch.tensor(R.MEAN)) / torch.tensor(R.STD)
        np.testing.assert_allclose(f32, t.numpy(), rtol=0, atol=1e-6)
        np.testing.assert_allclose(f32, R.normalize_u8_f64(u8), rtol=0, atol=1e-6)
        s2d = R.space_to_depth_ref(f32)
        assert s2d.shape == (B, (H + 1) // 2, (W + 1) // 2, 16)
        assert (s2d[..., 12:] == 0).all()
        for y in range(2 * s2d.shape[1]):
            for x in range(2 * s2d.shape[2]):
                c0 = ((y % 2) * 2 + (x % 2)) * 3
                want = f32[:, y, x] if (y < H and x < W) else np.zeros((B, 3), np.float32)
                assert np.array_equal(s2d[:, y // 2, x // 2, c0:c0 + 3], want)


@pytest.mark.parametrize('cols', R.L2_COLS)
def test_l2norm_ref_is_normalize(cols):
    for rows in R.L2_ROWS:
        x = R.l2_rows(rows, cols)
        np.testing.assert_allclose(F.normalize(torch.from_numpy(x), p=2, dim=1).numpy(), R.l2norm_ref(x), rtol=2e-6, atol=1e-7)
    z = np.zeros((2, cols), np.float32)
    assert (R.l2norm_ref(z) == 0).all()
    with np.errstate(invalid='ignore'):
        assert np.isnan(R.l2norm_ref(z, 0.0)).all()       # no eps: 0 / 0, as np.linalg.norm division gives in whiten_features
    if cols in (64, 256):
        u = R.unit_sign_rows(5, cols)
        assert np.array_equal(R.l2norm_ref(u), u.astype(np.float64) / np.sqrt(cols)) and np.sqrt(cols) in (8.0, 16.0)
    tiny = R.l2_rows(1, cols) * np.float32(1e-14)
    assert np.sqrt((tiny.astype(np.float64) ** 2).sum()) < 1e-12
    assert ((tiny == 0) | (tiny.astype(np.float32) ** 2 >= np.finfo(np.float32).tiny)).all()       # squares stay normal
    np.testing.assert_allclose(R.l2norm_ref(tiny), tiny.astype(np.float64) / 1e-12, rtol=1e-7)


@pytest.mark.parametrize('shape', R.MULTISCALE_SHAPES)
def test_multiscale_ref_is_the_oracle_pool(shape):
    import dir_oracle as O
    S, N, D = shape
    xi = R.multiscale_int_input(S, N, D)
    assert np.abs(xi).sum(axis=0).max() < 2 ** 24 and np.array_equal(xi, np.rint(xi))
    if S > 1:       # (the oracle, like the reference, returns a single scale as it is)
        np.testing.assert_allclose(O.pool(list(torch.from_numpy(xi)), 'mean').numpy(), R.multiscale_pool_ref(xi, 'mean'), rtol=2e-7)
    for p in (3.0, 2.5):
        x = R.multiscale_gem_input(S, N, D, p)
        flat = x.reshape(S, -1)
        assert (flat[:, R.MS_ZERO_COL] == 0).all() and (flat == 0).sum() > S + 1
        assert (np.abs(flat) == np.float32(1e-8)).sum() > 3 * S
        if S > 1:
            assert ((flat > 0).any(0) & (flat < 0).any(0)).mean() > 0.3          # signs mixed across scales
        assert R.multiscale_kappa(x, p).max() <= R.MULTISCALE_KAPPA
        ref = R.multiscale_pool_ref(x, 'gem', p)
        assert ref.reshape(-1)[R.MS_ZERO_COL] == 0.0
        np.testing.assert_allclose(ref.reshape(-1)[R.MS_TINY_COL], 1e-6 ** (1 / p), rtol=1e-6)     # the clamp, twice
        if S > 1:
            np.testing.assert_allclose(O.pool(list(torch.from_numpy(x)), 'gem', p).numpy(), ref, rtol=2e-5, atol=1e-6)


def _round_trips(x):
    t = torch.from_numpy(np.array(x))
    return all(torch.equal(t.to(dt).float(), t) for dt in (torch.bfloat16, torch.float16))


@pytest.mark.parametrize('hw', R.GLOBAL_SIZES)
def test_exact_inputs_are_exact(hw):
    """Integers in [-3, 7] are bf16 and fp16 numbers; summed (or clamped at 0 and cubed, then summed) over up to 1024 pixels
    they stay below 2^24 in magnitude whatever the grouping, so every fp32 partial sum is an integer held exactly."""
    H, W = hw
    for C in R.global_channels(H, W):
        for B in R.GLOBAL_BATCHES:
            x = R.int_map(B, H, W, C)
            assert _round_trips(x) and x.min() >= -3 and x.max() <= 7 and np.array_equal(x, np.rint(x))
            assert np.abs(x).sum(axis=(1, 2)).max() < 2 ** 24
            cubes = np.maximum(x.astype(np.float64), 0) ** 3
            assert cubes.sum(axis=(1, 2)).max() < 2 ** 24
            for c in R.nonpos_channels(C):
                assert x[..., c].max() <= 0
            if B > 1:
                assert not np.array_equal(x[0], x[1])
            if H * W > 8:
                assert not np.array_equal(x[..., 0], x[..., 1])
    if (H, W) == (32, 32):
        assert 7 ** 3 * 1024 < 2 ** 24          # the largest sum any case can form: 351232
    assert _round_trips(np.array([64.0, 0.0], np.float32)) and _round_trips(R.unit_sign_rows(5, 256))


def test_f32_entry_points_check_their_arguments_like_the_16_bit_ones():
    """No launch: every call here is refused on the host."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    m = (ctypes.c_float * 3)(0, 0, 0)
    assert lib.dir_prep_input_f32(None, 0, m, m, p, 1, 2, 2, None) == -1 and b'prep_input' in lib.dir_last_error()
    assert lib.dir_prep_input_f32(p, 0, m, m, p, 1, 0, 2, None) == -1
    assert lib.dir_prep_input_f32(p, 7, m, m, p, 1, 2, 2, None) == -1 and b'bad image format' in lib.dir_last_error()
    assert lib.dir_prep_input_f32(p, _lib.DIR_IMG_U8_NHWC, None, None, p, 1, 2, 2, None) == -1 and b'mean/std' in lib.dir_last_error()
    assert lib.dir_maxpool_3x3s2_f32(p, None, 1, 2, 2, 4, None) == -1 and b'maxpool' in lib.dir_last_error()
    assert lib.dir_maxpool_3x3s2_f32(p, p, 1, 2, 2, 6, None) == -1 and b'multiple of 4' in lib.dir_last_error()
    assert lib.dir_global_pool_f32(p, None, 1, 2, 2, 64, 0, 3.0, 1e-6, 0.0, None) == -1 and b'global_pool' in lib.dir_last_error()
    assert lib.dir_global_pool_f32(p, p, 1, 2, 2, 32, 0, 3.0, 1e-6, 0.0, None) == -1 and b'multiple of 64' in lib.dir_last_error()
    assert lib.dir_global_pool_f32(p, p, 1, 2, 2, 64, 0, 0.0, 1e-6, 0.0, None) == -1 and b'p <= 0' in lib.dir_last_error()
    assert lib.dir_global_pool_f32(p, p, 1, 2, 2, 64, 9, 3.0, 1e-6, 0.0, None) == -1 and b'bad pooling' in lib.dir_last_error()
    assert lib.dir_upsample_add_f32(p, p, None, 1, 2, 2, 1, 1, 4, None) == -1 and b'upsample_add' in lib.dir_last_error()
    assert lib.dir_upsample_add_f32(p, p, p, 1, 2, 2, 0, 1, 4, None) == -1
    assert lib.dir_upsample_add_f32(p, p, p, 1, 2, 2, 1, 1, 6, None) == -1 and b'multiple of 4' in lib.dir_last_error()

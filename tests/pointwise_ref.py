"""Inputs and references for the pointwise kernels (csrc/pointwise.hip and the fp32 twins at the end of csrc/conv_f32.hip):
global pooling, max-pool 3x3 s2, prep_input, upsample_add, row L2 norm and multi-scale pooling.

The references are plain numpy, fp64 wherever a bound is taken against them, each written from the operation's definition in
the reference project (dirtorch/nets/layers/pooling.py:38-40, dirtorch/nets/rmac_resnet.py:52-59, dirtorch/utils/common.py:41-55,
dirtorch/utils/transforms.py:617-623); tests/test_pointwise_ref_cpu.py pins them against the CPU oracle and torch's own
functions, and pins what the 'exact' inputs promise: values that bf16 and fp16 both hold, and sums whose every partial stays
below 2^24, so that an fp32 sum of them is the same number in any order.  tests/test_pointwise_gpu.py runs the kernels.
"""
import functools

import numpy as np
import torch

F32_EPS_GEM = float(np.float32(1e-6))      # the clamp as the kernels receive it (a float argument)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

# (H, W) of the global-pool cases: the 16-bit kernel walks pixels in rows of 32 lanes, 128 per trip (4 unrolled loads with a
# clamped tail), the fp32 twin in rows of 16
GLOBAL_SIZES = [(1, 1), (1, 31), (4, 8), (3, 11), (127, 1), (8, 16), (3, 43), (13, 20), (31, 33), (32, 32)]
GLOBAL_BATCHES = (1, 3)
MAXPOOL_SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (1, 9), (9, 1), (7, 12), (15, 9), (16, 16)]
PREP_SIZES = [(1, 1), (2, 3), (3, 2), (21, 18), (37, 41), (16, 48)]
UPSAMPLE_SHAPES = [(2, 7, 5, 4, 3, 64), (1, 14, 14, 7, 7, 256), (3, 9, 16, 5, 8, 8), (1, 64, 64, 32, 32, 1024),
                   (1, 29, 23, 10, 7, 4), (2, 5, 9, 5, 9, 8)]           # (B, H, W, h, w, C); the last is the identity size
L2_COLS = [1, 63, 64, 65, 255, 256, 257, 2048, 2051]
L2_ROWS = (1, 5)
MULTISCALE_SHAPES = [(1, 3, 70), (3, 1, 255), (3, 2, 128), (5, 7, 37), (2, 4, 2048)]      # (S, N, D)
MULTISCALE_KAPPA = 8.0      # sum |term| / |sum term| allowed in a gem column (see multiscale_gem_input)


def global_channels(H, W):
    """64 (one channel block), 192 (three), and the real 2048 at the real map size only."""
    return (64, 192, 2048) if (H, W) == (32, 32) else (64, 192)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


# ---- inputs -----------------------------------------------------------------------------------------------------------
def nonpos_channels(C):
    """Channels of int_map that hold no positive value: GeM of them is the clamp itself."""
    return (5, C - 1)


@functools.lru_cache(maxsize=None)
def int_map(B, H, W, C):
    """NHWC fp32 integers in [-3, 7], different per image, pixel and channel; the channels of nonpos_channels in [-3, 0]."""
    g = np.random.RandomState(1000 + 7 * H + 13 * W + C + 31 * B)
    x = g.randint(-3, 8, size=(B, H, W, C)).astype(np.float32)
    for c in nonpos_channels(C):
        x[..., c] = g.randint(-3, 1, size=(B, H, W))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def rand_map(B, H, W, C):
    """|N(0,1)| * 2 - 0.3, fp32 NHWC: mostly positive, some below the clamp (the inputs of test_ops_gpu.test_global_pool)."""
    g = torch.Generator().manual_seed(14 + 7 * H + 13 * W + C + 31 * B)
    x = (torch.randn(B, H, W, C, generator=g).abs() * 2 - 0.3).numpy()
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def signed_map(B, H, W, C):
    """N(0,1) fp32 NHWC with the first 64 channels of image 0 entirely negative: a zero-initialised accumulator, or a zero from
    padding, would win the max there."""
    g = torch.Generator().manual_seed(15 + 7 * H + 13 * W + C + 31 * B)
    x = torch.randn(B, H, W, C, generator=g).numpy()
    x[0, :, :, :64] = -np.abs(x[0, :, :, :64]) - 0.01
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def maxpool_map(B, H, W, C):
    """N(0,1) fp32 NHWC, the last image of the batch entirely negative."""
    g = torch.Generator().manual_seed(13 + 7 * H + 13 * W + C)
    x = torch.randn(B, H, W, C, generator=g).numpy()
    x[B - 1] = -np.abs(x[B - 1]) - 0.01
    x.setflags(write=False)
    return x


def u8_image(B, H, W):
    """uint8 NHWC.  Pixel n (row-major) of image b holds ((n + 17 b) * m_c + o_c) mod 256 in channel c with m_c odd: every
    channel of every image with at least 256 pixels contains every byte value, and the three channels differ."""
    n = np.arange(H * W, dtype=np.int64).reshape(1, H, W, 1) + 17 * np.arange(B, dtype=np.int64).reshape(B, 1, 1, 1)
    m = np.array([7, 11, 13], np.int64).reshape(1, 1, 1, 3)
    o = np.array([3, 101, 200], np.int64).reshape(1, 1, 1, 3)
    return ((n * m + o) % 256).astype(np.uint8)


def f32_image(B, H, W):
    """N(0,1) fp32 NCHW (an already normalised image)."""
    g = torch.Generator().manual_seed(12 + 7 * H + 13 * W + B)
    return torch.randn(B, 3, H, W, generator=g).numpy()


def upsample_inputs(shape):
    B, H, W, h, w, C = shape
    g = torch.Generator().manual_seed(H * 131 + w)
    return torch.randn(B, H, W, C, generator=g).numpy(), torch.randn(B, h, w, C, generator=g).numpy()


def l2_rows(rows, cols):
    g = torch.Generator().manual_seed(15 + rows * 4099 + cols)
    return torch.randn(rows, cols, generator=g).numpy()


def unit_sign_rows(rows, cols):
    """Rows of +1 / -1: with cols = 64 or 256 the norm is 8 or 16 and every output exactly +-2^-3 or +-2^-4."""
    g = np.random.RandomState(rows * 4099 + cols)
    return (g.randint(0, 2, size=(rows, cols)) * 2 - 1).astype(np.float32)


def multiscale_int_input(S, N, D):
    """fp32 integers in [-9, 9]."""
    g = np.random.RandomState(S * 100003 + N * 1009 + D)
    return g.randint(-9, 10, size=(S, N, D)).astype(np.float32)


# columns (of the flattened N*D axis) that multiscale_gem_input plants
MS_ZERO_COL, MS_ONE_LIVE_COL, MS_TINY_COL, MS_TINY_MIXED_COL, MS_TINY_AND_NORMAL_COL = 0, 1, 2, 3, 4


def multiscale_gem_input(S, N, D, p):
    """[S,N,D] fp32, N(0, 0.5^2) with signs mixed across the scales, and planted: an all-zero column, a column that is zero in
    every scale but the last, a column of +1e-8 (below the 1e-6 clamp), one of +-1e-8, one that mixes 1e-8 with ordinary
    values, and single zeros and +-1e-8 sprinkled through the rest.

    sign(acc) * max(|acc|, 1e-6)^(1/p) jumps at acc = 0, and acc is a signed sum: where the terms cancel, rounding decides
    the sign and no tolerance can hold.  So a column whose condition number sum|t_s| / |sum t_s| (t_s = sympow(x_s, p), in
    fp64) exceeds MULTISCALE_KAPPA gets one sign throughout.  A powf good to 2 ulps then moves acc by at most
    2 * 2^-24 * KAPPA relative and the result by 1/p of that: 4e-7 at KAPPA = 8, p = 2.5, fifty times inside rtol = 2e-5."""
    g = np.random.RandomState(S * 100003 + N * 1009 + D + int(p * 10))
    x = (g.standard_normal((S, N * D)) * 0.5).astype(np.float32)
    j = np.arange(N * D)
    x[j % S, j] = np.where(j % 7 == 5, 0.0, x[j % S, j])
    x[(j + 1) % S, j] = np.where(j % 11 == 3, np.where(j % 2 == 0, 1e-8, -1e-8), x[(j + 1) % S, j])
    x[:, MS_ZERO_COL] = 0.0
    x[:-1, MS_ONE_LIVE_COL] = 0.0
    x[-1, MS_ONE_LIVE_COL] = -0.75
    x[:, MS_TINY_COL] = 1e-8
    x[:, MS_TINY_MIXED_COL] = np.where(np.arange(S) % 2 == 0, 1e-8, -1e-8)
    x[:, MS_TINY_AND_NORMAL_COL] = np.where(np.arange(S) % 2 == 0, 0.375, -1e-8)
    t = _sympow64(x.astype(np.float64), float(np.float32(p)))
    bad = np.abs(t).sum(0) > MULTISCALE_KAPPA * np.abs(t.sum(0))
    x[:, bad] = np.abs(x[:, bad])
    return x.reshape(S, N, D)


def multiscale_kappa(x, p):
    """sum|t_s| / |sum t_s| of every column with a non-zero term (fp64)."""
    x = _np(x).astype(np.float64)
    t = _sympow64(x.reshape(x.shape[0], -1), float(np.float32(p)))
    num, den = np.abs(t).sum(0), np.abs(t.sum(0))
    live = num > 0
    return num[live] / den[live]


# ---- references -------------------------------------------------------------------------------------------------------
def center_mask_ref(cb, H, W):
    """1 + the 4x4 mask with cb in its middle 2x2, upsampled bilinearly with align_corners=True to H x W (rmac_resnet.py:52-56);
    fp64 [H,W].  An axis of one output pixel samples source index 0, where the mask is 0."""
    m = np.zeros((4, 4))
    m[1:3, 1:3] = cb

    def axis(n):
        s = np.arange(n) * 3.0 / (n - 1) if n > 1 else np.zeros(n)
        i0 = np.minimum(np.floor(s).astype(np.int64), 2)
        return i0, s - i0
    y0, fy = axis(H)
    x0, fx = axis(W)
    top = m[y0][:, x0] * (1 - fx) + m[y0][:, x0 + 1] * fx
    bot = m[y0 + 1][:, x0] * (1 - fx) + m[y0 + 1][:, x0 + 1] * fx
    return 1 + top * (1 - fy)[:, None] + bot * fy[:, None]


def global_pool_ref(x, mode, p=3.0, eps=F32_EPS_GEM, cb=0.0):
    """NHWC [B,H,W,C] -> fp64 [B,C]: (x * mask) then max / mean / (mean(clamp(x, eps)^p))^(1/p) over H*W (pooling.py:38-40,
    rmac_resnet.py:52-59).  p and eps are taken as the fp32 numbers the kernels receive."""
    x = _np(x).astype(np.float64)
    if cb > 0:
        x = x * center_mask_ref(float(np.float32(cb)), x.shape[1], x.shape[2])[None, :, :, None]
    if mode == 'max':
        return x.max(axis=(1, 2))
    if mode == 'avg':
        return x.sum(axis=(1, 2)) / (x.shape[1] * x.shape[2])
    p = float(np.float32(p))
    return (np.maximum(x, float(np.float32(eps))) ** p).mean(axis=(1, 2)) ** (1.0 / p)


def maxpool_ref(x):
    """MaxPool2d(3, stride 2, padding 1) on NHWC (resnet.py:119): out[ph, pw] = max over rows 2 ph - 1 + r, columns
    2 pw - 1 + s (r, s in 0..2) that exist.  Same dtype as x."""
    x = _np(x)
    B, H, W, C = x.shape
    PH, PW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = np.full((B, 2 * PH + 1, 2 * PW + 1, C), -np.inf, x.dtype)
    pad[:, 1:H + 1, 1:W + 1] = x
    out = np.full((B, PH, PW, C), -np.inf, x.dtype)
    for r in range(3):
        for s in range(3):
            out = np.maximum(out, pad[:, r:r + 2 * PH:2, s:s + 2 * PW:2])
    return out


def space_to_depth_ref(nhwc):
    """[B,H,W,3] -> [B,ceil(H/2),ceil(W/2),16]: channel (dy*2+dx)*3 + c = pixel (2 y2 + dy, 2 x2 + dx) channel c; channels
    12..15 and the row / column an odd size lacks are zero.  Same dtype."""
    v = _np(nhwc)
    B, H, W, _ = v.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2
    out = np.zeros((B, H2, W2, 16), v.dtype)
    for dy in range(2):
        for dx in range(2):
            sub = v[:, dy::2, dx::2]
            c0 = (dy * 2 + dx) * 3
            out[:, :sub.shape[1], :sub.shape[2], c0:c0 + 3] = sub
    return out


def normalize_u8_f32(u8, mean=MEAN, std=STD):
    """ToTensor then Normalize (transforms.py:617-623) in fp32, operation by operation: ((u / 255) - mean) / std, NHWC."""
    u = _np(u8).astype(np.float32)
    return ((u / np.float32(255.0)) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)


def normalize_u8_f64(u8, mean=MEAN, std=STD):
    """The same in fp64, from the fp32 mean / std the kernel receives."""
    u = _np(u8).astype(np.float64)
    return ((u / 255.0) - np.asarray(mean, np.float32).astype(np.float64)) / np.asarray(std, np.float32).astype(np.float64)


def nearest_index(n_out, n_in):
    """Source index of F.interpolate(mode='nearest', size=...): min(floor(dst * (float32)(in / out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def upsample_add_ref(x, low):
    """x + nearest-upsampled low, NHWC (rmac_resnet_fpn.py:55-60), in the dtype of x (one add)."""
    x, low = _np(x), _np(low)
    ys, xs = nearest_index(x.shape[1], low.shape[1]), nearest_index(x.shape[2], low.shape[2])
    return x + low[:, ys][:, :, xs]


def l2norm_ref(x, eps=1e-12):
    """x / max(||x||_2, eps) per row (F.normalize; rmac_resnet.py:7-9), fp64; eps as the fp32 number the kernel receives."""
    x = _np(x).astype(np.float64)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    with np.errstate(invalid='ignore'):        # eps = 0 and a zero row: 0 / 0 = NaN is the answer
        return x / np.maximum(n, float(np.float32(eps)))


def _sympow64(x, p, eps=F32_EPS_GEM):
    s = np.sign(x)
    return np.maximum(x * s, eps) ** p * s


def multiscale_pool_ref(x, pooling, p=3.0):
    """common.pool (common.py:41-55) of the stacked [S,N,D] scales, fp64 (without the reference's single-scale shortcut, which
    the kernel does not take either): the mean, or sympow(mean(sympow(x, p)), 1/p) with sympow(x, p) = sign(x) max(|x|, 1e-6)^p."""
    x = _np(x).astype(np.float64)
    if pooling == 'mean':
        return x.sum(axis=0) / x.shape[0]
    p = float(np.float32(p))
    return _sympow64(_sympow64(x, p).mean(axis=0), 1.0 / p)


# ---- measures ---------------------------------------------------------------------------------------------------------
def ulps_f32(got, ref64):
    """|got - ref| in units of the fp32 spacing at ref (fp64 arrays in, fp64 out)."""
    got, ref64 = _np(got).astype(np.float64), np.asarray(ref64, np.float64)
    return np.abs(got - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def max_excess(got, ref64, rtol, atol):
    """max of |got - ref| / (atol + rtol |ref|): assert_allclose passes iff this is <= 1."""
    got, ref64 = _np(got).astype(np.float64), np.asarray(ref64, np.float64)
    return float(np.max(np.abs(got - ref64) / (atol + rtol * np.abs(ref64))))

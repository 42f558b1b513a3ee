"""Operands that overflow fp16 at chosen stores - and nowhere else - with the expected non-finite positions worked out by the
fp32 / fp64 CPU reference of the same rounded operands.  Shared by test_overflow_plant_cpu.py (the preconditions: the
reference's non-finite set is exactly what the plant intends) and test_overflow_word_gpu.py (the kernels' overflow word and
their own outputs against those sets).

Everything here is CPU torch.  A case is a dict of named operand tensors (the last two of a kind are cached: treat them as read-only) plus `edits`, a
list of (operand name, index tuple, value); `planted` clones what it edits.  A position is (m, n): m the flattened output
pixel ((b * OH + oh) * OW + ow), n the output channel; a non-finite set is a frozenset of such pairs.

The single plant: x = 256 at the pixel the centre filter tap of output pixel m reads, channel c0 = (7 m + 3 n) mod Cin, and
w[n, centre, c0] = +-1024: one product of +-2^18, four times fp16's largest finite value (65504) and a finite fp32 / bf16
number.  Every other output sees at most 256 * |w| or 1024 * |x| with |w| < 1 and |x| < 6 beside its clean |y| <= ~9."""
import functools

import torch
import torch.nn.functional as F

from test_ops_gpu import CONV_SHAPES, DTYPES, DUAL_SHAPES, SEAM_SHAPES, SPLITK_SHAPES, _rand, conv_reference

X_PLANT, W_PLANT = 256.0, 1024.0
F16_MAX = 65504.0
# rows with more input pixels than this take their expected set from the library's plain device checker, not from the CPU
CPU_REFERENCE_PIXELS = 20000
SHAPE_BY_NAME = {s[0]: s for s in CONV_SHAPES}
SHAPE_BY_NAME.update({'splitk/' + s[0]: s for s in SPLITK_SHAPES})
SEAM_PLANES = [(64, 64), (128, 128), (64, 128)]
STEM_SIZES = [(37, 41), (30, 23)]
UPSAMPLE_SHAPES = [(2, 7, 5, 4, 3, 64), (1, 14, 14, 7, 7, 256), (3, 9, 16, 5, 8, 8)]      # test_heads_gpu's, without its 8 MB one


def small(shape):
    return shape[1] * shape[2] * shape[3] <= CPU_REFERENCE_PIXELS


def geom(shape):
    """(B, H, W, Cin, Cout, k, stride, pad, use_res, relu, OH, OW, M) of a CONV_SHAPES / SPLITK_SHAPES row"""
    _, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    return B, H, W, Cin, Cout, k, stride, pad, use_res, relu, OH, OW, B * OH * OW


def positions(M, N):
    """The five planted positions: the corners of the [M, N] output matrix and one interior element off every tile edge."""
    return [(0, 0), (M - 1, N - 1), (M - 1, 0), (0, N - 1), (M // 2, N // 2 + 1)]


def nonfinite(t16):
    """frozenset of (m, n) where a [..., N] tensor is inf or NaN"""
    t = t16.reshape(-1, t16.shape[-1])
    return frozenset((int(i), int(j)) for i, j in (~torch.isfinite(t.float())).nonzero().tolist())


def planted(case, edits):
    """A copy of the case with the edits applied (only the edited tensors are cloned)."""
    out = dict(case)
    for name, idx, value in edits:
        if out[name] is case[name]:
            out[name] = case[name].clone()
        out[name][idx] = value
    return out


def plant_on_device(dev, edits):
    """The same edits on a dict of device tensors, in place -> the list that undoes them (apply it with this function too)."""
    undo = []
    for name, idx, value in edits:
        undo.append((name, idx, dev[name][idx].item()))
        dev[name][idx] = value
    return undo[::-1]


# ---- the plain convolution (dir_conv_bn_act, dir_conv_bn_act_splitk) -----------------------------------------------------
@functools.lru_cache(maxsize=2)
def conv_case(name, dname):
    """test_conv_variant_vs_oracle's operands of a shape row: the same seeds and scales"""
    B, H, W, Cin, Cout, k, stride, pad, use_res, relu, OH, OW, M = geom(SHAPE_BY_NAME[name])
    dt = DTYPES[dname]
    return {'x': _rand((B, H, W, Cin), 1).to(dt), 'w': _rand((Cout, k, k, Cin), 2, (2.0 / (k * k * Cin)) ** 0.5).to(dt),
            'bias': _rand((Cout,), 3, 0.2), 'res': _rand((B, OH, OW, Cout), 4).to(dt) if use_res else None}


def _centre_pixel(shape, m):
    """index (b, ih, iw) of the input pixel the centre tap (pad, pad) of output pixel m reads"""
    B, H, W, Cin, Cout, k, stride, pad, use_res, relu, OH, OW, M = geom(shape)
    b, r = divmod(m, OH * OW)
    oh, ow = divmod(r, OW)
    assert oh * stride < H and ow * stride < W
    return b, oh * stride, ow * stride


def conv_single(shape, m, n, sign=1):
    Cin, pad = shape[4], shape[8]
    c0 = (7 * m + 3 * n) % Cin
    return [('x', _centre_pixel(shape, m) + (c0,), X_PLANT), ('w', (n, pad, pad, c0), sign * W_PLANT)]


def cancel_channels(m, n, Cin):
    """c0 of the single plant and a different channel c1 of the last 64-channel K slice"""
    c0 = (7 * m + 3 * n) % Cin
    span = min(64, Cin)
    c1 = Cin - span + (c0 % span + span // 2) % span
    assert c1 != c0
    return c0, c1


def conv_cancelling(shape, m, n):
    """+2^18 through c0 and -2^18 through c1 into the same output: partial sums four times above fp16's range, a finite sum"""
    pad = shape[8]
    c0, c1 = cancel_channels(m, n, shape[4])
    px = _centre_pixel(shape, m)
    return [('x', px + (c0,), X_PLANT), ('w', (n, pad, pad, c0), W_PLANT), ('x', px + (c1,), X_PLANT), ('w', (n, pad, pad, c1), -W_PLANT)]


def conv_plants(shape, every_sign=False):
    """[(m, n, sign, edits, intended non-finite set)]: the five positions with +1024, (0, 0) - or with every_sign all five -
    with -1024 too.  Intended: {(m, n)}, but nothing for -1024 under a ReLU, which comes before the pack."""
    M, Cout, relu = geom(shape)[12], shape[5], shape[10]
    out = []
    for i, (m, n) in enumerate(positions(M, Cout)):
        for sign in ((1, -1) if every_sign or i == 0 else (1,)):
            out.append((m, n, sign, tuple(conv_single(shape, m, n, sign)), frozenset() if sign < 0 and relu else frozenset([(m, n)])))
    return out


def conv_cancel_positions(shape):
    p = positions(geom(shape)[12], shape[5])
    return [p[0], p[1], p[4]]


def conv_output(shape, case):
    return conv_reference(case['x'], case['w'], case['bias'], case['res'], shape[7], shape[8], shape[10])


@functools.lru_cache(maxsize=None)
def conv_expected(name, dname, edits):
    """non-finite set of the reference's output rounded to the storage format (edits: a tuple, for the cache)"""
    shape = SHAPE_BY_NAME[name]
    return nonfinite(conv_output(shape, planted(conv_case(name, dname), edits)).to(DTYPES[dname]))


def conv_boundary(shape, m, n, bias_n):
    """fp16, all zero but one x = 1, w[n, centre, c0] = 65504 and bias[n]: y[m, n] = 65504 + bias[n] exactly, in fp32 and in any
    order.  No ReLU; rows whose variants exist only with a residual get one of zeros."""
    B, H, W, Cin, Cout, k, stride, pad, use_res, relu, OH, OW, M = geom(shape)
    c0 = (7 * m + 3 * n) % Cin
    case = {'x': torch.zeros(B, H, W, Cin, dtype=torch.float16), 'w': torch.zeros(Cout, k, k, Cin, dtype=torch.float16),
            'bias': torch.zeros(Cout), 'res': torch.zeros(B, OH, OW, Cout, dtype=torch.float16) if use_res else None}
    case['x'][_centre_pixel(shape, m) + (c0,)] = 1.0
    case['w'][n, pad, pad, c0] = F16_MAX
    case['bias'][n] = bias_n
    return case


# ---- the fused seams (dir_conv_c3c1 and its _keep / _ds / _wpair forms) ------------------------------------------------
@functools.lru_cache(maxsize=2)
def seam_case(B, H, W, P, P2, dname, form='plain'):
    """form 'plain': test_fused_seam_vs_oracle_and_two_kernel_path's operands; 'ds': test_fused_seam_with_downsample_as_extra_k's
    (P = P2 = 64, x and wcat = [w3 | wds] instead of res); 'wp' / 'ds_wp' (fp16): the same with lo planes of 1/64 the size for
    w3 (wcat), w1 and, in 'ds_wp', the block input x."""
    dt = DTYPES[dname]
    c = {'t2': F.relu(_rand((B, H, W, P), 1)).to(dt), 'w1': _rand((P2, 4 * P), 5, (2.0 / (4 * P)) ** 0.5).to(dt), 'b1': _rand((P2,), 6, 0.2)}
    w3 = _rand((4 * P, P), 2, (2.0 / P) ** 0.5).to(dt)
    if form in ('ds', 'ds_wp'):
        assert P == 64 and P2 == 64
        c['x'] = F.relu(_rand((B, H, W, 64), 7)).to(dt)
        c['w3'] = torch.cat([w3, _rand((256, 64), 8, (2.0 / 64) ** 0.5).to(dt)], dim=1).contiguous()
        c['b3'] = _rand((256,), 3, 0.2) + _rand((256,), 9, 0.2)
    else:
        c['w3'], c['b3'] = w3, _rand((4 * P,), 3, 0.2)
        c['res'] = F.relu(_rand((B, H, W, 4 * P), 4)).to(dt)
    if form in ('wp', 'ds_wp'):
        assert dname == 'fp16'
        c['w3_lo'] = (_rand(tuple(c['w3'].shape), 12, (2.0 / P) ** 0.5) / 64).to(dt)
        c['w1_lo'] = (_rand((P2, 4 * P), 15, (2.0 / (4 * P)) ** 0.5) / 64).to(dt)
    if form == 'ds_wp':
        c['x_lo'] = (_rand((B, H, W, 64), 17) / 64).to(dt)
    return c


def seam_reference(case, dname, relu3, relu1=True):
    """(y, t1) in the storage format: conv3 (+ residual or downsample as extra K) in fp32, rounded, then conv1 of the ROUNDED y"""
    dt = DTYPES[dname]
    rows = lambda t: t.float().reshape(-1, t.shape[-1])      # noqa: E731
    w3 = case['w3'].float() + (case['w3_lo'].float() if 'w3_lo' in case else 0)
    if 'x' in case:
        y = rows(case['t2']) @ w3[:, :64].T + rows(case['x']) @ w3[:, 64:].T + case['b3']
        if 'x_lo' in case:      # the kernel forms wds_hi . x_lo and drops lo x lo
            y = y + rows(case['x_lo']) @ case['w3'].float()[:, 64:].T
    else:
        y = rows(case['t2']) @ w3.T + case['b3'] + rows(case['res'])
    y16 = (F.relu(y) if relu3 else y).to(dt)
    w1 = case['w1'].float() + (case['w1_lo'].float() if 'w1_lo' in case else 0)
    t1 = y16.float() @ w1.T + case['b1']
    return y16, (F.relu(t1) if relu1 else t1).to(dt)


def _pix(m, H, W):
    b, r = divmod(m, H * W)
    return (b,) + divmod(r, W)


def seam_plant_y(case, m, n, sign=1):
    """y[m, n] = +-2^18 through t2 and conv3's weight (conv1 then reads the stored inf: the whole row m of t1 follows)"""
    B, H, W, P = case['t2'].shape
    c0 = (7 * m + 3 * n) % P
    return [('t2', _pix(m, H, W) + (c0,), X_PLANT), ('w3', (n, c0), sign * W_PLANT)]


def seam_plant_t1(case, m, n2):
    """t1[m, n2] = 2^18 with y finite: y[m, c] is about 256 (through the residual; in the downsample forms through x and a unit
    weight of the downsample half) and w1[n2, c] = 1024"""
    B, H, W, P = case['t2'].shape
    c = (7 * m + 3 * n2) % (4 * P)
    if 'x' in case:
        cx = (5 * m + n2) % 64
        first = [('x', _pix(m, H, W) + (cx,), X_PLANT), ('w3', (c, 64 + cx), 1.0)]
    else:
        first = [('res', _pix(m, H, W) + (c,), X_PLANT)]
    return first + [('w1', (n2, c), W_PLANT)]


def _stored(ey, H, W, keep_stride):
    if keep_stride <= 1:
        return ey
    return frozenset((m, n) for m, n in ey if _pix(m, H, W)[1] % keep_stride == 0 and _pix(m, H, W)[2] % keep_stride == 0)


def seam_expected(case, dname, relu3, keep_stride=0):
    """(non-finite set of y as stored, of t1); with keep_stride = s only the pixels on rows and columns that are multiples of s
    are stored - the others keep what the caller put there, which the tests make finite"""
    y16, t1 = seam_reference(case, dname, relu3)
    return _stored(nonfinite(y16), case['t2'].shape[1], case['t2'].shape[2], keep_stride), nonfinite(t1)


@functools.lru_cache(maxsize=None)
def _seam_sets(key, edits, relu3):
    y16, t1 = seam_reference(planted(seam_case(*key), edits), key[5], relu3)
    return nonfinite(y16), nonfinite(t1)


def seam_expected_of(key, edits, relu3, keep_stride=0):
    """seam_expected of seam_case(*key) with the edits, the reference computed once per (key, edits, relu3)"""
    ey, et = _seam_sets(key, tuple(edits), relu3)
    return _stored(ey, key[1], key[2], keep_stride), et


# ---- the two-source GEMM (dir_conv_dual) ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def dual_case(B, OH, OW, Cin, Cout, Cin2, s2, dname):
    """test_conv3_plus_downsample_as_one_two_source_gemm's operands"""
    dt = DTYPES[dname]
    H2, W2 = (OH - 1) * s2 + 1 + (s2 - 1), (OW - 1) * s2 + 1
    w3, wds = _rand((Cout, Cin), 2, (2.0 / Cin) ** 0.5).to(dt), _rand((Cout, Cin2), 8, (2.0 / Cin2) ** 0.5).to(dt)
    return {'t2': F.relu(_rand((B, OH, OW, Cin), 1)).to(dt), 'x': F.relu(_rand((B, H2, W2, Cin2), 7)).to(dt),
            'wcat': torch.cat([w3, wds], dim=1).contiguous(), 'bias': _rand((Cout,), 3, 0.2) + _rand((Cout,), 9, 0.2)}


def dual_plant(case, s2, m, n, source, sign=1):
    """+-2^18 into y[m, n] through the first source (t2) or the second (the strided block input x)"""
    B, OH, OW, Cin = case['t2'].shape
    b, oh, ow = _pix(m, OH, OW)
    if source == 0:
        c = (7 * m + 3 * n) % Cin
        return [('t2', (b, oh, ow, c), X_PLANT), ('wcat', (n, c), sign * W_PLANT)]
    c = (7 * m + 3 * n) % case['x'].shape[3]
    return [('x', (b, oh * s2, ow * s2, c), X_PLANT), ('wcat', (n, Cin + c), sign * W_PLANT)]


def dual_cancelling(case, s2, m, n):
    """+2^18 through the first source, -2^18 through the second (the last K slices)"""
    return dual_plant(case, s2, m, n, 0) + dual_plant(case, s2, m, n, 1, -1)


def dual_expected(case, s2, dname, relu):
    Cin = case['t2'].shape[3]
    Cout = case['wcat'].shape[0]
    w = case['wcat']
    y = (conv_reference(case['t2'], w[:, :Cin].reshape(Cout, 1, 1, -1), case['bias'], None, 1, 0, False) +
         conv_reference(case['x'], w[:, Cin:].reshape(Cout, 1, 1, -1), torch.zeros(Cout), None, s2, 0, False))
    return nonfinite((F.relu(y) if relu else y).to(DTYPES[dname]))


@functools.lru_cache(maxsize=None)
def _dual_set(key, edits, s2, relu):
    return dual_expected(planted(dual_case(*key), edits), s2, key[7], relu)


def dual_expected_of(key, edits, s2, relu):
    """dual_expected of dual_case(*key) with the edits, the reference computed once"""
    return _dual_set(key, tuple(edits), s2, relu)


# ---- the paired forms (dir_conv_bn_act_pair, dir_conv_pair_dual): fp16 (hi, lo) planes, the word is judged on hi --------
def split_pair(t):
    hi = t.to(torch.float16)
    return hi, (t - hi.float()).to(torch.float16)


@functools.lru_cache(maxsize=2)
def pair_case(geom_row):
    """test_pair_conv_vs_torch_fp32's operands (GEOMS row: B, H, W, Cin, Cout, k, stride, pad, residual, relu), NHWC planes"""
    B, H, W, Cin, Cout, k, stride, pad, with_res, relu = geom_row
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (k * k * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g)
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    c = {'bias': bias}
    c['x_hi'], c['x_lo'] = split_pair(x.permute(0, 2, 3, 1).contiguous())
    c['w_hi'], c['w_lo'] = split_pair(w.permute(0, 2, 3, 1).contiguous())
    if with_res:
        c['res_hi'], c['res_lo'] = split_pair(torch.randn(B, Cout, OH, OW, generator=g).permute(0, 2, 3, 1).contiguous())
    return c


def pair_plant(geom_row, m, n, sign=1):
    B, H, W, Cin, Cout, k, stride, pad, with_res, relu = geom_row
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    b, oh, ow = _pix(m, OH, OW)
    c0 = (7 * m + 3 * n) % Cin
    xi, wi = (b, oh * stride, ow * stride, c0), (n, pad, pad, c0)
    return [('x_hi', xi, X_PLANT), ('x_lo', xi, 0.0), ('w_hi', wi, sign * W_PLANT), ('w_lo', wi, 0.0)]


def pair_expected(geom_row, case):
    """non-finite set of the hi plane: fp16 of the fp64 convolution of the joined (hi + lo) operands"""
    B, H, W, Cin, Cout, k, stride, pad, with_res, relu = geom_row
    j = lambda a, b: (a.double() + b.double()).permute(0, 3, 1, 2)      # noqa: E731
    y = F.conv2d(j(case['x_hi'], case['x_lo']), j(case['w_hi'], case['w_lo']), case['bias'].double(), stride, pad)
    if with_res:
        y = y + j(case['res_hi'], case['res_lo'])
    return nonfinite((F.relu(y) if relu else y).permute(0, 2, 3, 1).to(torch.float16))


PAIR_DUAL_SHAPES = [(2, 16, 24, 64, 256), (1, 9, 13, 64, 128), (1, 7, 9, 128, 256)]      # test_pair_conv_dual_equals_...'s


@functools.lru_cache(maxsize=2)
def pair_dual_case(B, H, W, C, Cout):
    g = torch.Generator().manual_seed(31)
    t2, x = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    w3, wd = torch.randn(Cout, C, generator=g) / C ** 0.5, torch.randn(Cout, C, generator=g) / C ** 0.5
    c = {'bias': torch.randn(Cout, generator=g) + torch.randn(Cout, generator=g)}
    c['t2_hi'], c['t2_lo'] = split_pair(t2.permute(0, 2, 3, 1).contiguous())
    c['x_hi'], c['x_lo'] = split_pair(x.permute(0, 2, 3, 1).contiguous())
    c['w_hi'], c['w_lo'] = split_pair(torch.cat([w3, wd], dim=1).contiguous())
    return c


def pair_dual_plant(case, m, n, source, sign=1):
    B, H, W, C = case['t2_hi'].shape
    c0 = (7 * m + 3 * n) % C
    xi, wi = _pix(m, H, W) + (c0,), (n, c0 + source * C)
    act = 't2' if source == 0 else 'x'
    return [(act + '_hi', xi, X_PLANT), (act + '_lo', xi, 0.0), ('w_hi', wi, sign * W_PLANT), ('w_lo', wi, 0.0)]


def pair_dual_expected(case, relu):
    C = case['t2_hi'].shape[3]
    rows = lambda a, b: (a.double() + b.double()).reshape(-1, a.shape[-1])      # noqa: E731
    w = case['w_hi'].double() + case['w_lo'].double()
    y = rows(case['t2_hi'], case['t2_lo']) @ w[:, :C].T + rows(case['x_hi'], case['x_lo']) @ w[:, C:].T + case['bias'].double()
    return nonfinite((F.relu(y) if relu else y).to(torch.float16))


# ---- the stems: conv 7x7 s2 p3 + ReLU + max-pool 3x3 s2 p1; the pool spreads one inf over the windows that hold it --------
@functools.lru_cache(maxsize=2)
def stem_case(H, W):
    """test_fused_stem_pool_vs_conv_relu_maxpool's operands, in fp32 (the test rounds them to the storage format)"""
    return {'img': _rand((2, 3, H, W), 23), 'w7': _rand((64, 3, 7, 7), 24, (2.0 / (49 * 64)) ** 0.5 * 3), 'bias': _rand((64,), 25, 0.1)}


def stem_plant(b, oh, ow, n, ch=1, sign=1):
    """conv output (b, oh, ow, n) = +-2^18: the image pixel under the centre tap (3, 3) of that output, one colour channel"""
    return [('img', (b, ch, 2 * oh, 2 * ow), X_PLANT), ('w7', (n, ch, 3, 3), sign * W_PLANT)]


def pool_windows(b, oh, ow, n, OH, OW):
    """the pooled positions (3x3 stride 2 pad 1) whose window holds conv pixel (b, oh, ow), channel n: one to four"""
    PH, PW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    return frozenset(((b * PH + ph) * PW + pw, n) for ph in range(PH) for pw in range(PW) if abs(2 * ph - oh) <= 1 and abs(2 * pw - ow) <= 1)


def stem_expected(case, dname):
    """one storage plane (dir_stem_pool)"""
    dt = DTYPES[dname]
    conv = F.relu(F.conv2d(case['img'].to(dt).float(), case['w7'].to(dt).float(), case['bias'], 2, 3))
    return nonfinite(F.max_pool2d(conv.to(dt).float(), 3, 2, 1).permute(0, 2, 3, 1).to(dt))


def stem_pair_expected(case, acc=torch.float64):
    """(hi, lo) planes of image and filter (dir_stem_pool_pair): fp64 (acc: or fp32, for a large image) of the joined operands,
    judged on the hi plane"""
    j = lambda t: sum(p.to(acc) for p in split_pair(t))      # noqa: E731
    conv = F.relu(F.conv2d(j(case['img']), j(case['w7']), case['bias'].to(acc), 2, 3))
    return nonfinite(F.max_pool2d(conv.to(torch.float16).to(acc), 3, 2, 1).permute(0, 2, 3, 1).to(torch.float16))


U8_MEAN, U8_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
U8_GREY = (124, 116, 104)      # 255 * mean to the nearest byte: the normalised image is within 0.002 of zero


@functools.lru_cache(maxsize=2)
def stem_u8_case(B, H, W):
    """dir_stem_pool_u8 folds ToTensor + Normalize into the filter: the patch it multiplies is u / 256 < 1 and a folded weight
    must itself fit fp16, so ONE tap cannot reach 65504.  The plant is a white pixel on a grey image (normalised: 2.2 .. 2.6
    on ~0) under the three colour taps of the centre, each folded weight 60000: the conv output is about 99000 at that
    pixel and within a few hundred of the bias everywhere else."""
    g = torch.Generator().manual_seed(31)
    u8 = torch.tensor(U8_GREY, dtype=torch.uint8).repeat(B, H, W, 1).contiguous()
    return {'u8': u8, 'w': torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5, 'scale': 0.5 + torch.rand(64, generator=g),
            'bias': 0.3 * torch.randn(64, generator=g)}


def stem_u8_plant(case, b, oh, ow, n, sign=1):
    edits = [('u8', (b, 2 * oh, 2 * ow, ch), 255) for ch in range(3)]
    folded = 60000.0
    return edits + [('w', (n, ch, 3, 3), sign * folded * 255.0 * U8_STD[ch] / (256.0 * float(case['scale'][n]))) for ch in range(3)]


def stem_u8_expected(case, acc=torch.float64):
    """fp64 (acc: or fp32, for a large image) of the reference's own arithmetic (tests/test_stem_u8_gpu.py reference_stem),
    judged on the hi plane"""
    x = (case['u8'].to(acc) / 255.0 - torch.tensor(U8_MEAN).to(acc)) / torch.tensor(U8_STD).to(acc)
    y = F.conv2d(x.permute(0, 3, 1, 2), case['w'].to(acc), None, 2, 3) * case['scale'].to(acc).view(1, -1, 1, 1) + case['bias'].to(acc).view(1, -1, 1, 1)
    return nonfinite(F.max_pool2d(F.relu(y).to(torch.float16).to(acc), 3, 2, 1).permute(0, 2, 3, 1).to(torch.float16))


# ---- upsample_add: y = x + nearest-upsampled low ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def upsample_case(B, H, W, h, w, C, dname):
    """test_upsample_add_matches_interpolate's operands"""
    g = torch.Generator().manual_seed(H * 131 + w)
    x = torch.randn(B, H, W, C, generator=g).to(DTYPES[dname])
    return {'x': x, 'low': torch.randn(B, h, w, C, generator=g).to(DTYPES[dname])}


def upsample_plant(case, m, n, value=40000.0):
    """x = low = 40000 at element (m, n) and at its source: 80000 in one place, 40000 + noise wherever else the source lands"""
    B, H, W, C = case['x'].shape
    h, w = case['low'].shape[1:3]
    b, Y, X = _pix(m, H, W)
    idx = torch.arange(h * w, dtype=torch.float32).reshape(1, 1, h, w)
    sy, sx = divmod(int(F.interpolate(idx, size=(H, W), mode='nearest')[0, 0, Y, X]), w)
    return [('x', (b, Y, X, n), value), ('low', (b, sy, sx, n), value)]


def upsample_expected(case, dname):
    H, W = case['x'].shape[1:3]
    up = F.interpolate(case['low'].float().permute(0, 3, 1, 2), size=(H, W), mode='nearest')
    return nonfinite((case['x'].float() + up.permute(0, 2, 3, 1)).to(DTYPES[dname]))

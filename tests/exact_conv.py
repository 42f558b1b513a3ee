"""Operands on which fp32 summation is exact in every order, and the zero-tolerance conv reference built on them (a helper
module like synth.py / picker_cases.py; tests/test_exact_lattice_cpu.py checks the claims below on the CPU,
tests/test_exact_conv_gpu.py and tests/test_exact_tuner_candidates_gpu.py use them on the device).

The lattice: activations in {0, 1, 2, 3}; filter taps in {-2 ... 2}, scaled by 2^-6 on the odd input channels; the fp32 bias a
multiple of 2^-6 (even output channels) or of 2^-7 ... 2^-10 (odd ones, fine_frac()) with |bias| <= 32; the residual an integer
in [-128, 128].  Activations, taps and residual are exact in bf16 and in fp16.  For K = R S Cin <= 4 608 every partial sum of
every subset of the terms is a multiple of 2^-7 of magnitude <= 6 K + 160 <= 27 808 < 2^15: at most 22 significant bits, exact in
fp32 with two bits to spare.  (With integer taps only the bias would carry fraction bits and the K slices of a split-K launch
would hold small integers, which 16 bits hold exactly: a slice that passes through 16 bits would go unseen.  Measured on the
MI355X with such a mutant: 15 of 27 648 elements differed with integer taps.)  So ANY association - MFMA block order, split-K slices, two-source K, rotated K walks - forms
the same fp32 number, the one rounding left is the 16-bit store, and

    expected = RNE_dtype(act(exact_sum + bias + res))        compared bit for bit.

A kernel that truncates where it should round, rounds a partial result to 16 bits, or adds a term after the rounding instead
of before it differs in a large share of the outputs (the bias' six fraction bits make 45-95 % of the positive outputs inexact
in the target format and 4-26 % exact ties), where a relative tolerance sees nothing.  bit_budget() is the proof obligation:
pure arithmetic on the shape, asserted wherever operands are drawn.  The fused seam has a lattice of its own (seam_operands).

Row of a plain convolution: (tag, B, H, W, Cin, Cout, k, stride, pad, residual, relu) - picker_cases' row without the launch.
"""
import ctypes
import math
import zlib

import torch
import torch.nn.functional as F

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16}

X_MAX = 3            # activations 0 ... 3
W_MAX = 2            # taps -2 ... 2 on the even input channels ...
W_FRAC = 6           # ... and (-2 ... 2) x 2^-6 on the odd ones: every partial sum carries fraction bits, not only the bias
RES_MAX = 128        # residual: an integer of magnitude <= 128
BIAS_MAX = 32        # |bias| <= 32 ...
BIAS_FRAC = 6        # ... a multiple of 2^-6 on the even channels ...
SUM_BITS = 22        # ... and of 2^-f on the odd ones, f = fine_frac(): as fine as keeps every sum within 22 significant bits

FP16_MAX = 65504.0
FP16_MIN_NORMAL = 2.0 ** -14

# per form: the fraction bits of each operand class (value = integer x 2^-frac).  'conv': one store.  'seam' / 'seam_ds'
# (conv_c3c1, conv_c3c1_ds): y = act(t2 . w3 + b3 (+ res)) is rounded to the dtype and conv1 multiplies the ROUNDED y, so y has to
# stay an integer (a 16-bit rounding of an integer is an integer; with 2^-6 fractions in b3 fp16 would keep them and conv1's sums
# would need 26 bits): b3 an integer, w1 taps {-2 ... 2} x 2^-seam_w1_frac(), b1 as lattice_bias() draws it for conv1's sums.
def seam_w1_frac(y_max, P):
    """Fraction bits of w1's taps: the coarsest scale that keeps conv1's largest possible sum of the rounded y, bias included,
    inside fp16's range (4 at planes 128, 3 at planes 64; with 2^-5 everywhere t1 stays so small at planes 64 that fp16 has
    to round under 30 % of it - measured on the CPU reference, 18-26 %)."""
    f = 0
    while y_max * W_MAX * 4 * P * 2.0 ** -f + BIAS_MAX >= FP16_MAX:
        f += 1
    return f



def fine_frac(mag):
    """Fraction bits of the bias on the odd channels, for sums of magnitude <= mag: 7 at the longest K of a ResNet (K = 4 608,
    |sum| < 2^15: 22 bits, two to spare in fp32), up to 10 where K is short.  Why two depths: with 2^-6 alone a K = 64 sum (|value| ~ 20) is
    inexact in fp16 in only 14 % of the positive outputs (measured on the CPU reference; fp16 holds 2^-6 up to 32), so a wrong
    fp16 rounding would show in few elements; with 2^-10 alone bf16 would meet an exact tie in under 1 %.  Even channels keep the
    ties, odd channels the inexact fp16 values; test_exact_lattice_cpu.py asserts both shares for every row."""
    return max(BIAS_FRAC, min(10, SUM_BITS - int(mag).bit_length()))


def lattice_bias(n, mag, g, device):
    """fp32 [n]: |bias| <= 32, a multiple of 2^-6 on even channels and of 2^-fine_frac(mag) on odd ones."""
    f = fine_frac(mag)
    coarse = _ints((n,), -(BIAS_MAX << BIAS_FRAC), BIAS_MAX << BIAS_FRAC, g, device).float() * 2.0 ** -BIAS_FRAC
    fine = _ints((n,), -(BIAS_MAX << f), BIAS_MAX << f, g, device).float() * 2.0 ** -f
    odd = (torch.arange(n, device=device) % 2 == 1)
    return torch.where(odd, fine, coarse)


def lattice_weights(shape, g, device):
    """fp32 [..., Cin]: taps -2 ... 2, times 2^-W_FRAC on the odd input channels (exact in bf16 and fp16)."""
    w = _ints(shape, -W_MAX, W_MAX, g, device).float()
    odd = (torch.arange(shape[-1], device=device) % 2 == 1)
    return torch.where(odd, w * 2.0 ** -W_FRAC, w)


def out_hw(H, W, k, stride, pad):
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


def _audit(points):
    """points: [(where, largest magnitude, resolution)].  Every value formed there is a multiple of `resolution` of at most that
    magnitude: it must fit fp32's 24 significant bits, stay inside fp16's range, and not reach below fp16's normal numbers."""
    out = []
    for where, mag, res in points:
        bits = int(mag / res).bit_length()
        assert bits <= 24, '%s: multiples of 2^%d up to %g need %d significant bits (fp32 holds 24)' % (where, _log2(res), mag, bits)
        assert mag < FP16_MAX, '%s: magnitude %g reaches fp16 overflow' % (where, mag)
        assert res >= FP16_MIN_NORMAL, '%s: resolution %g is below the smallest normal fp16' % (where, res)
        out.append((where, mag, res, bits))
    return out


def _log2(v):
    return int(round(math.log2(v)))


def bit_budget(row, form='conv'):
    """[(where, largest possible magnitude, resolution, significant bits)] at every point where a kernel of `form` adds; asserts
    bits <= 24, magnitude < 65 504 and resolution >= 2^-14 at each.  Forms: 'conv' (row of a plain convolution; the two-source
    GEMM and the stem are plain convolutions of their total K), 'seam' (B, H, W, P, P2, K3) with K3 the K of the first GEMM
    (P, or P + 64 for the downsample form, which has no residual)."""
    if form == 'conv':
        tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = row[:11]
        K = k * k * Cin
        s = X_MAX * W_MAX * K
        r = 2.0 ** -fine_frac(s + BIAS_MAX + RES_MAX)
        return _audit([('products summed in any order, K = %d' % K, s, 2.0 ** -W_FRAC),
                       ('sum + bias', s + BIAS_MAX, r),
                       ('sum + bias + residual', s + BIAS_MAX + (RES_MAX if use_res else 0), r)])
    if form == 'seam':
        B, H, W, P, P2, K3, use_res = row
        y = X_MAX * W_MAX * K3 + BIAS_MAX + (RES_MAX if use_res else 0)           # an integer: b3 and the residual are integers
        rw = 2.0 ** -seam_w1_frac(y, P)
        t = y * W_MAX * rw * 4 * P                                                # RNE(y) is an integer of magnitude <= y
        return _audit([('conv3: products + b3 + residual, K = %d' % K3, y, 1.0),
                       ('conv1: products of the rounded y, K = %d' % (4 * P), t, rw),
                       ('conv1: sum + b1', t + BIAS_MAX, min(rw, 2.0 ** -fine_frac(t + BIAS_MAX)))])
    raise ValueError(form)


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _ints(shape, lo, hi, g, device):
    """Uniform integers lo ... hi as int8 / int16 (no 8-byte temporaries: the largest operands have 5 x 10^8 elements)."""
    dt = torch.int8 if -128 <= lo and hi <= 127 else torch.int16 if -32768 <= lo and hi <= 32767 else torch.int32
    return torch.randint(lo, hi + 1, shape, generator=g, device=device, dtype=dt)


def row_seed(row):
    return zlib.crc32(str(row[0]).encode())


def lattice_operands(row, dtype, device='cpu', seed=None):
    """x [B,H,W,Cin], w [Cout,k,k,Cin] (16-bit), bias fp32 [Cout], res [B,OH,OW,Cout] or None of a plain-conv row, drawn from the
    lattice on `device` from a seeded generator: the same values for both dtypes.  Asserts the row's bit budget."""
    bit_budget(row)
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = row[:11]
    g = _gen(device, row_seed(row) if seed is None else seed)
    OH, OW = out_hw(H, W, k, stride, pad)
    x = _ints((B, H, W, Cin), 0, X_MAX, g, device).to(dtype)
    w = lattice_weights((Cout, k, k, Cin), g, device).to(dtype)
    bias = lattice_bias(Cout, X_MAX * W_MAX * k * k * Cin + BIAS_MAX + RES_MAX, g, device)
    res = _ints((B, OH, OW, Cout), -RES_MAX, RES_MAX, g, device).to(dtype) if use_res else None
    return x, w, bias, res


def exact_value(x, w, bias, res, stride, pad, relu, precision=torch.float32):
    """act(conv(x, w) + bias (+ res)) of NHWC / [Cout,R,S,Cin] operands on the CPU in `precision`, NHWC, BEFORE the store's
    rounding.  On lattice operands fp32 is exact (test_exact_lattice_cpu.py: equal to fp64 bit for bit)."""
    xc = x.to('cpu', precision).permute(0, 3, 1, 2)
    wc = w.to('cpu', precision).permute(0, 3, 1, 2)
    y = F.conv2d(xc, wc, bias.to('cpu', precision), stride, pad)
    if res is not None:
        y = y + res.to('cpu', precision).permute(0, 3, 1, 2)
    if relu:
        y = F.relu(y)
    return y.permute(0, 2, 3, 1).contiguous()


def exact_reference(x, w, bias, res, stride, pad, relu, dtype):
    """(expected 16-bit NHWC tensor, its fp32 value before the rounding): torch's .to(dtype) rounds to nearest even."""
    v = exact_value(x, w, bias, res, stride, pad, relu)
    return v.to(dtype), v


def seam_reference(t2, w3, b3, res, w1, b1, relu3, relu1, dtype, x=None):
    """The fused seam's chain with its documented storage point: y = RNE(act3(t2 . w3 (+ x . wds) + b3 (+ res))), t1 =
    RNE(act1(y . w1 + b1)) - conv1 reads the ROUNDED y.  w3 is [4P, K3] over [t2 ; x] when x is given.
    Returns (y, t1, y value, t1 value)."""
    src = t2 if x is None else torch.cat([t2, x], dim=3)
    vy = exact_value(src, w3.reshape(w3.shape[0], 1, 1, -1), b3, res, 1, 0, relu3)
    y = vy.to(dtype)
    vt = exact_value(y, w1.reshape(w1.shape[0], 1, 1, -1), b1, None, 1, 0, relu1)
    return y, vt.to(dtype), vy, vt


def seam_operands(shape, dtype, device='cpu', seed=0, ds=False):
    """Lattice operands of conv_c3c1 (t2, w3, b3, res, w1, b1) or, ds=True, of conv_c3c1_ds (t2, x, wcat, bias, w1, b1):
    shape = (B, H, W, P, P2).  Asserts the seam's bit budget."""
    B, H, W, P, P2 = shape
    bit_budget((B, H, W, P, P2, 2 * P if ds else P, not ds), 'seam')
    g = _gen(device, seed)
    t2 = _ints((B, H, W, P), 0, X_MAX, g, device).to(dtype)
    w3 = _ints((4 * P, 2 * P if ds else P), -W_MAX, W_MAX, g, device).to(dtype)
    b3 = _ints((4 * P,), -BIAS_MAX, BIAS_MAX, g, device).float()
    other = (_ints((B, H, W, P), 0, X_MAX, g, device) if ds else _ints((B, H, W, 4 * P), -RES_MAX, RES_MAX, g, device)).to(dtype)
    y_max = X_MAX * W_MAX * (2 * P if ds else P) + BIAS_MAX + (0 if ds else RES_MAX)
    rw = 2.0 ** -seam_w1_frac(y_max, P)
    w1 = (_ints((P2, 4 * P), -W_MAX, W_MAX, g, device).float() * rw).to(dtype)
    b1 = lattice_bias(P2, y_max * W_MAX * rw * 4 * P + BIAS_MAX, g, device)
    return t2, w3, b3, other, w1, b1


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def mismatch_report(got, want, what, BM=64, BN=64, value=None, resolution=2.0 ** -10):
    """None when `got` and `want` (16-bit tensors [..., Cout], any device) agree bit for bit; otherwise the text of the finding:
    how many elements differ and in how many (m // BM, n // BN) tiles, the first (pixel row m, channel n) with its tile, got /
    want as values and as bit patterns, and - when `value`, the fp32 number before the store's rounding, is given - got - value
    in units of `resolution` (2^-10, the finest bias fraction, unless the caller knows better): a whole number of 2^10 units there
    names the missing or doubled product, a fraction a term that went through a rounding."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    C = got.shape[-1]
    if torch.equal(got, want):        # (values: +0 == -0, and a NaN - which the lattice cannot produce - equals nothing)
        return None
    g2, w2 = _bits(got).reshape(-1, C), _bits(want).reshape(-1, C)
    bad = (g2 != w2) & ~((got.reshape(-1, C) == 0) & (want.reshape(-1, C) == 0))
    n_bad = int(bad.sum())
    idx = bad.nonzero()
    m, n = (int(v) for v in idx[0])
    head = idx[:100000]
    tiles = len(torch.unique((head[:, 0] // BM) * (1 << 20) + head[:, 1] // BN))
    mask = 0xffff if got.element_size() == 2 else 0xffffffff
    gv, wv = float(got.reshape(-1, C)[m, n].float()), float(want.reshape(-1, C)[m, n].float())
    msg = ('%s: %d / %d elements differ in their bits; first at m = %d, n = %d, tile (%d, %d) of %d x %d: got %r (0x%x) want %r '
           '(0x%x); %d tiles hold differing elements (of the first 100 000)'
           % (what, n_bad, bad.numel(), m, n, m // BM, n // BN, BM, BN, gv, int(g2[m, n]) & mask, wv, int(w2[m, n]) & mask, tiles))
    if value is not None:
        v = float(value.reshape(-1, C)[m, n])
        msg += '; the fp32 value before the store is %r: got - value = %g lattice units of 2^%d' % (v, (gv - v) / resolution,
                                                                                                   _log2(resolution))
    return msg


def report_mismatch(got, want, row, BM=64, BN=64, value=None, resolution=2.0 ** -10):
    """Fail (AssertionError carrying mismatch_report's text) unless got == want bit for bit."""
    msg = mismatch_report(got, want, row if isinstance(row, str) else str(row[0]), BM, BN, value, resolution)
    assert msg is None, msg


def rounding_stats(value, dtype):
    """(share of outputs that are positive, share of the positive outputs that the dtype cannot hold, share of the positive
    outputs that are exact ties) of an fp32 tensor of pre-store values."""
    v = value.reshape(-1).double()
    pos = v[v > 0]
    r = pos.float().to(dtype).double()
    inexact = r != pos
    # a tie: the two neighbours of the value in the target format are equally far.  The neighbour on the other side of `pos`
    # from r is r -/+ one ulp (values far from a power of two; at a binade edge the tie test only under-counts)
    ulp = 2.0 ** (torch.floor(torch.log2(pos)) - (7 if dtype == torch.bfloat16 else 10))
    tie = inexact & ((r - pos).abs() * 2 == ulp)
    n = max(int(pos.numel()), 1)
    return float(pos.numel()) / max(int(v.numel()), 1), float(inexact.sum()) / n, float(tie.sum()) / n


def stat_crop(row):
    """The row's layer at batch 1 on a map of at most 40 x 40: the distribution of its outputs does not depend on the map (every
    output pixel away from the border sums the same K lattice terms), so the conditions on the reference are checked there."""
    tag, B, H, W = row[:4]
    return (tag, 1, min(H, 40), min(W, 40)) + tuple(row[4:11])


# ---- the rows of the small-shape tests (tests/test_exact_conv_gpu.py) ---------------------------------------------------------
NAIVE_ROW = ('naive_3x3_s2_res', 2, 10, 9, 64, 64, 3, 2, 1, True, True)
ANCHOR_ROW = ('anchor_1x1_k256_res', 2, 12, 11, 256, 128, 1, 1, 0, True, True)      # 264 pixels: three tiles of 128, the last ragged
STEM_SIZES = [(37, 41), (64, 64), (30, 23), (224, 131), (9, 120), (1024, 400)]       # test_fused_stem_pool_vs_conv_relu_maxpool's
SEAM_PLANES = [(64, 64), (128, 128), (64, 128)]
DUAL_EXTRA = [(2, 64, 64, 128, 512, 256, 2), (3, 33, 47, 256, 1024, 512, 2), (4, 96, 128, 128, 512, 256, 2)]


def dual_shapes():
    """(B, OH, OW, Cin, Cout, Cin2, stride2): the shapes test_conv3_plus_downsample_as_one_two_source_gemm runs."""
    from test_ops_gpu import DUAL_SHAPES
    return list(DUAL_SHAPES) + DUAL_EXTRA


def dual_row(shape):
    """The two-source GEMM as the plain 1x1 convolution of its concatenated K (bit budget, statistics)."""
    B, OH, OW, Cin, Cout, Cin2, s2 = shape
    return ('dual_%dx%dx%d_k%d+%d' % (B, OH, OW, Cin, Cin2), B, OH, OW, Cin + Cin2, Cout, 1, 1, 0, False, True)


def stem_row(hw, B=2):
    """The stem as the 7 x 7 stride-2 convolution of the 3-channel image (K = 147) it is."""
    return ('stem_%dx%d' % hw, B, hw[0], hw[1], 3, 64, 7, 2, 3, False, True)


def f32_rows():
    from test_strict_gpu import GEOMS
    return [('f32_%dx%dx%dx%d-%d-k%ds%d' % g[:7],) + tuple(g) for g in GEOMS]


def small_plain_rows():
    """Every plain-convolution row of the small-shape tests, the fused forms that are one convolution included."""
    from test_ops_gpu import CONV_SHAPES, SPLITK_SHAPES
    return (list(CONV_SHAPES) + list(SPLITK_SHAPES) + [NAIVE_ROW, ANCHOR_ROW] + [dual_row(s) for s in dual_shapes()] +
            [stem_row(hw) for hw in STEM_SIZES] + f32_rows())


def seam_cases():
    """(B, H, W, P, P2, ds) of conv_c3c1 (ds False) and conv_c3c1_ds (True) on test_ops_gpu.SEAM_SHAPES."""
    from test_ops_gpu import SEAM_SHAPES
    return ([(B, H, W, P, P2, False) for B, H, W in SEAM_SHAPES for P, P2 in SEAM_PLANES] +
            [(B, H, W, 64, 64, True) for B, H, W in SEAM_SHAPES])


# ---- every launch the tuner can keep -----------------------------------------------------------------------------------------
def _query(fn, variant, shape):
    from dirtorch_amd import _lib
    B, H, W, Cin, Cout, k, stride, pad, use_res = shape[:9]
    OH, OW = out_hw(H, W, k, stride, pad)
    out = ctypes.c_int()
    _lib.call(fn, variant, B, H, W, Cin, Cout, k, k, stride, pad, OH, OW, int(use_res), ctypes.byref(out))
    return out.value


def variant_admissible(variant, shape):
    """dir_conv_variant_admissible for shape = (B, H, W, Cin, Cout, k, stride, pad, residual, ...): host-only."""
    return bool(_query('dir_conv_variant_admissible', variant, shape))


def variant_splitk(variant, shape):
    """dir_conv_variant_splitk: the number of K slices the tuner launches an admissible variant in (1 = no split)."""
    return _query('dir_conv_variant_splitk', variant, shape)


def workload_shapes():
    """{(B, H, W, Cin, Cout, k, stride, pad, residual, relu): 'workload.layer' of its first occurrence} over
    picker_cases.workload_layers()."""
    from picker_cases import workload_layers
    out = {}
    for l in workload_layers():
        out.setdefault(tuple(l[2:]), '%s.%s' % l[:2])
    return out


def layer_kind(shape):
    B, H, W, Cin, Cout, k, stride, pad, use_res = shape[:9]
    return (Cin, Cout, k, stride, use_res)


def _pixels(shape):
    B, H, W, Cin, Cout, k, stride, pad = shape[:8]
    OH, OW = out_hw(H, W, k, stride, pad)
    return B * OH * OW


def _ragged(shape, tag):
    """A native-size or multiscale map whose output does not divide into the kernels' pixel tiles (8 x 32, 16 x 32, rows of 64 /
    256 pixels)."""
    B, H, W, Cin, Cout, k, stride, pad = shape[:8]
    OH, OW = out_hw(H, W, k, stride, pad)
    return tag.startswith(('native_', 'ms')) and OH % 16 != 0 and OW % 32 != 0 and (B * OH * OW) % 256 != 0


def candidate_table(middle=True):
    """The tuner's candidate launches on the claimed workloads, COMPUTED from the library's own predicates.

    A class is (layer kind (Cin, Cout, k, stride, residual), variant) admissible on some shape of workload_layers().  Returns
    (classes, rows, unlaunchable):
      classes       {class: [shapes it is admissible on]}
      rows          {shape: (tag, sorted variant indices to launch there)} - for every class its admissible shape with the fewest
                    output pixels, the one with the most, one ragged native / multiscale shape when it admits one (middle=True),
                    and one shape for every distinct (class, split factor > 1)
      unlaunchable  [(class, shape)] admissible pairs conv_launch would refuse for their size (picker_cases.launchable): a
                    disagreement between the predicate and the launch, which the CPU test reports
    Shapes already chosen for another class are preferred, so that the distinct shapes (operands, naive launches) stay few."""
    from dirtorch_amd import ops
    from picker_cases import launchable
    names = ops.conv_variant_names()
    shapes = workload_shapes()
    classes, splits, unlaunchable = {}, {}, []
    for sh in sorted(shapes):
        for v in range(len(names)):
            if not variant_admissible(v, sh):
                continue
            cls = layer_kind(sh) + (v,)
            if not launchable(*sh[:8]):
                unlaunchable.append((cls, sh))
                continue
            classes.setdefault(cls, []).append(sh)
            ks = variant_splitk(v, sh)
            if ks > 1:
                splits.setdefault(cls + (ks,), []).append(sh)
    rows = {}

    def take(sh, v):
        rows.setdefault(sh, set()).add(v)

    order = lambda sh: (_pixels(sh), sh)
    for cls, shs in sorted(classes.items()):
        take(min(shs, key=order), cls[-1])
        take(max(shs, key=order), cls[-1])
    for pool, wanted in ((splits, None), (classes, _ragged)) if middle else ((splits, None),):
        for key, shs in sorted(pool.items()):
            v = key[5]
            shs = [s for s in shs if wanted is None or wanted(s, shapes[s])]
            if not shs:
                continue
            have = [s for s in shs if s in rows]
            take(min(have or shs, key=order), v)
    return classes, {sh: (shapes[sh], sorted(vs)) for sh, vs in sorted(rows.items())}, unlaunchable


def table_row(shape, tag):
    """The plain-conv row (tag, B, H, W, Cin, Cout, k, stride, pad, residual, relu) of a candidate_table shape."""
    return ('wl.' + tag,) + tuple(shape)

"""The PAIR lattice: fp16 (hi, lo) operands on which every fp32 sum a paired kernel can form is exact in every order, its bit
budget and the fp64 references of the paired kernels (a helper module like exact_conv.py, which it builds on;
tests/test_exact_pair_cpu.py checks the claims below on the CPU, tests/test_exact_pair_gpu.py uses them on the device).

The arithmetic, as csrc/conv_pair.hip, csrc/conv_c3c1.hip and csrc/stem_u8.hip document it, stated here in fp64:

    convolution   v = sum(w_hi.x_hi + w_hi.x_lo + w_lo.x_hi) + bias (+ res_hi (+ res_lo)), ReLU; w_lo.x_lo is not formed;
                  x_lo = 0 for a single-plane x
    pair output   hi = RNE_fp16(v), lo = RNE_fp16(v - hi) of the fp32 v; fp16 subnormals kept
    seam          y = RNE_fp16(act3(sum (w3_hi + w3_lo).t2 + b3 + res)); downsample form: sum (w_hi + w_lo).t2 +
                  sum (wd_hi + wd_lo).x_hi + sum wd_hi.x_lo + b; t1 = RNE_fp16(relu(sum (w1_hi + w1_lo).y + b1)) of the ROUNDED y
    stem          split(maxpool3x3s2(relu(conv7x7s2(pair image, pair filter) + bias))), pooled in fp32

The lattice (kind 'std'): x_hi in {0 ... 3}, x_lo in {-1, 0, 1} x 2^-4; w_hi in {-2 ... 2}, w_lo in {-1, 0, 1} x 2^-7; res_hi an
integer in +-128, res_lo in {-8 ... 8} x 2^-7; the bias |b| <= 32, a multiple of 2^-7 on the even output channels and of 2^-f
on the odd ones, f = 24 - bit_length(largest possible |sum|).  The lo planes are deliberately NOT <= 2^-11 |hi|: the kernels
multiply whatever planes they are given, and a lost or misplaced lo product is then many lattice units, not a fraction of one.

Bits used.  One term is at most 6 + 2/16 + 3/128 on the 2^-7 grid, so K terms, the bias' +-32 and the residual's +-(128 + 1/16)
stay below 2^13 up to K = 1 152 (the longest row here): 20 significant bits on the EVEN output channels, four to spare in fp32
(the conv lattice of exact_conv.py keeps two).  The ODD channels spend all 24 on purpose, and no row can keep spare bits there: a
pair holds 11 + 1 + 11 bits, so only a value that needs (nearly) all of fp32's 24 makes lo carry eleven significant bits - on
a 22-bit lattice a kernel whose lo plane lost its last bits would go unseen.  Even so an ordinary row never makes lo ROUND
(hi + lo == v in 100 % of its outputs: sums of random signs stay far below the worst case), nor go subnormal.  Two extra kinds
do:
  'top'     1x1, K = 64, x_hi in {0, 1}, w_hi in {-1, 0, 1}, the same lo planes, a bias of either sign with 150 <= |b| <= 180 on
            the 2^-16 grid, no ReLU: every output is a 23- or 24-bit number in (64, 256), 24 bits at every add, none spare; lo
            itself rounds in 24 % of the outputs (hi + lo != v).
  'scaled'  a 'std' row with the weight pair and the bias multiplied by 2^-12 (a power of two scales every sum exactly; the bit
            count is the 'std' row's): outputs of ~2^-9, w_lo an fp16 SUBNORMAL on input (2^-19), lo a subnormal on output.
  'stem'    the stem's filter goes through pack_stem_weight + split_pair, so the fp32 tap w = a + s 2^-12 (a in {-2 ... 2}, s in
            {-1, 0, 1}, s = 0 where a = 0) must split into exactly (a, s 2^-12): it does (|s 2^-12| is at most half an fp16 ulp
            of a, and the tie goes to the even a); K = 147: 22 bits for the products, 24 on the odd channels' 2^-14 bias grid.
The seams (w3, w1 pairs; 'seam_wp', 'seam_ds_wp'): conv1 multiplies the ROUNDED y, so y has to stay on a grid fp16 holds
exactly at its magnitude: w3_lo in {-1, 0, 1} x 2^-1 and integer b3 / residual give half-integers of magnitude <= 640 < 1 024;
the downsample form's x_lo and w_lo in {-1, 0, 1} give integers <= 1 312 < 2 048.  w1_hi in {-2 ... 2} x 2^-3 (2^-4 downsample
form: exact_conv.seam_w1_frac), w1_lo in {-1, 0, 1} three bits finer, b1 as lattice_bias draws it: conv1's sums are multiples
of 2^-7 below 44 700, 23 bits, one to spare.

bit_budget() is the proof obligation - pure arithmetic on the shape, asserted wherever operands are drawn: at most 24
significant bits at every add, every magnitude below 65 504, every input plane on fp16's grid (lo planes: multiples of 2^-24,
the subnormal spacing).

Row of a paired convolution: (tag, B, H, W, Cin, Cout, k, stride, pad, residual, relu, kind).
"""
import collections

import torch
import torch.nn.functional as F

import exact_conv as E
from exact_conv import _ints, out_hw, report_mismatch, row_seed      # noqa: F401  (re-exported: the pair tests' one import)

XL_FRAC = 4              # x_lo in {-1, 0, 1} x 2^-4
RES_LO_MAX = 8           # res_lo in {-8 ... 8} x 2^-7
BIAS_FRAC = 7            # bias on the even channels: multiples of 2^-7
TOP_BIAS = (150, 180)    # kind 'top': 150 <= |bias| <= 180 ...
TOP_BIAS_FRAC = 16       # ... on the 2^-16 grid
SCALE_EXP = -12          # kind 'scaled': weight pair and bias x 2^-12
FP16_SUBNORMAL = 2.0 ** -24

# per kind: largest x_hi, largest |w_hi|, fraction bits of w_lo, exponent of the power of two on weights and bias
Lat = collections.namedtuple('Lat', 'x_max w_max wl_frac scale_exp')
LATTICES = {'std': Lat(E.X_MAX, E.W_MAX, 7, 0), 'top': Lat(1, 1, 7, 0), 'scaled': Lat(E.X_MAX, E.W_MAX, 7, SCALE_EXP),
            'stem': Lat(E.X_MAX, E.W_MAX, 12, 0)}


def _audit(points):
    """exact_conv._audit where its floor (fp16's smallest NORMAL number) applies; the 'top' and 'scaled' kinds go below it on
    purpose and keep the other two conditions: 24 significant bits, magnitude under 65 504."""
    if all(res >= E.FP16_MIN_NORMAL for _, _, res in points):
        return E._audit(points)
    out = []
    for where, mag, res in points:
        bits = int(mag / res).bit_length()
        assert bits <= 24, '%s: multiples of 2^%d up to %g need %d significant bits (fp32 holds 24)' % (where, E._log2(res), mag, bits)
        assert mag < E.FP16_MAX, '%s: magnitude %g reaches fp16 overflow' % (where, mag)
        out.append((where, mag, res, bits))
    return out


def _planes(planes):
    """planes: [(name, largest magnitude, grid)] of fp16 INPUT planes: each value must be an fp16 number - a multiple of 2^-24
    (subnormals are kept), at most 11 significant bits, inside the range."""
    for name, mag, grid in planes:
        assert grid >= FP16_SUBNORMAL, '%s: multiples of 2^%d are below fp16\'s subnormal spacing 2^-24' % (name, E._log2(grid))
        assert int(mag / grid).bit_length() <= 11 and mag < E.FP16_MAX, '%s: %g on the 2^%d grid is not an fp16 number' % (name, mag, E._log2(grid))


def _sum_mag(K, lat, use_res, bias_max=E.BIAS_MAX):
    """Largest possible |sum| of a row in units of its scale: K terms of three products, the bias, the residual pair."""
    term = lat.w_max * lat.x_max + lat.w_max * 2.0 ** -XL_FRAC + lat.x_max * 2.0 ** -lat.wl_frac
    return K * term, K * term + bias_max + ((E.RES_MAX + RES_LO_MAX * 2.0 ** -7) if use_res else 0)


def fine_frac(mag):
    """Fraction bits of the bias on the odd output channels: all of fp32's 24 bits at the largest possible |sum|."""
    return 24 - int(mag).bit_length()


def seam_wp_geometry(ds):
    """(fraction bits of y's grid, largest |y|, fraction bits of w1_hi's scale) of the paired-weight seam (planes 64)."""
    if ds:      # t2 . (w_hi + w_lo) + x_hi . (wd_hi + wd_lo) + x_lo . wd_hi + b: every lo plane an integer
        yf, y_max = 0, 128 * E.X_MAX * (E.W_MAX + 1) + 64 * E.W_MAX + E.BIAS_MAX
    else:       # t2 . (w3_hi + w3_lo) + b3 + res: w3_lo half-integers
        yf, y_max = 1, 64 * E.X_MAX * (E.W_MAX + 0.5) + E.BIAS_MAX + E.RES_MAX
    return yf, y_max, E.seam_w1_frac(y_max * (1 + 2.0 ** -4), 64)      # (w1_hi + w1_lo <= 2 (1 + 2^-4) w1's scale)


def _pair_points(K, kind, use_res, bias_max):
    """The audited points of a paired convolution of K terms per output (bit_budget's 'pair' form)."""
    lat = LATTICES[kind]
    sc = 2.0 ** lat.scale_exp
    prod, total = _sum_mag(K, lat, use_res, bias_max)
    grid = 2.0 ** -max(lat.wl_frac, XL_FRAC)
    fine = min(grid, 2.0 ** -(TOP_BIAS_FRAC if kind == 'top' else max(fine_frac(total), BIAS_FRAC)))
    _planes([('x_hi', lat.x_max, 1.0), ('x_lo', 2.0 ** -XL_FRAC, 2.0 ** -XL_FRAC), ('w_hi', lat.w_max * sc, sc),
             ('w_lo', 2.0 ** -lat.wl_frac * sc, 2.0 ** -lat.wl_frac * sc), ('res_hi', E.RES_MAX, 1.0),
             ('res_lo', RES_LO_MAX * 2.0 ** -7, 2.0 ** -7)])
    return _audit([('three products per term summed in any order, K = %d' % K, prod * sc, grid * sc),
                   ('sum + bias', (prod + bias_max) * sc, fine * sc),
                   ('sum + bias + residual pair', total * sc, fine * sc)])


def bit_budget(row, form='pair'):
    """[(where, largest possible magnitude, resolution, significant bits)] at every point where a kernel of `form` adds.
    'pair': a row of a paired convolution (conv_pair_dual and the paired stem are paired convolutions of their total K);
    'pair_dual': (B, H, W, C, Cout) - 'pair' of K = 2 C with both biases, and the two-launch leg: the downsample's own output must
    be a value a pair holds EXACTLY (hi 11 bits, lo the remainder in 11 more) for the two paths to meet bit for bit;
    'seam_wp' / 'seam_ds_wp': (B, H, W, P2, w1 is a pair).  Any other form is exact_conv.bit_budget's."""
    if form == 'pair':
        tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
        assert not (use_res and LATTICES[kind].scale_exp), 'the residual pair is not scaled'
        return _pair_points(k * k * Cin, kind, use_res, TOP_BIAS[1] if kind == 'top' else E.BIAS_MAX)
    if form == 'pair_dual':
        B, H, W, C, Cout = row
        out = _pair_points(2 * C, 'std', False, 2 * E.BIAS_MAX)
        fine = out[-1][2]
        ds = _sum_mag(C, LATTICES['std'], False)[1]
        e = int(ds).bit_length()
        assert e + BIAS_FRAC <= 22, 'the downsample pair cannot hold multiples of 2^-7 up to %g exactly' % ds
        return out + _audit([('two launches: downsample + its bias (a pair holds it exactly: %d + 7 bits)' % e, ds, 2.0 ** -BIAS_FRAC),
                             ('two launches: conv3 + b3 + the downsample pair as residual', 2 * ds, fine)])
    if form in ('seam_wp', 'seam_ds_wp'):
        B, H, W, P2, w1_pair = row
        yf, y_max, f1 = seam_wp_geometry(form == 'seam_ds_wp')
        assert y_max < 2.0 ** (11 - yf), 'fp16 does not hold multiples of 2^-%d up to %g' % (yf, y_max)
        rw = 2.0 ** -f1
        w1_max = E.W_MAX * rw + (rw / 8 if w1_pair else 0)
        res = 2.0 ** -yf * (rw / 8 if w1_pair else rw)
        t = y_max * w1_max * 256
        _planes([('w3_lo / x_lo', 1.0, 2.0 ** -yf), ('w1_hi', E.W_MAX * rw, rw), ('w1_lo', rw / 8, rw / 8)])
        return _audit([('conv3 (+ downsample): products + bias (+ residual), on fp16\'s grid', y_max, 2.0 ** -yf),
                       ('conv1: products of the rounded y, K = 256', t, res),
                       ('conv1: sum + b1', t + E.BIAS_MAX, min(res, 2.0 ** -E.fine_frac(t + E.BIAS_MAX)))])
    return E.bit_budget(row, form)


def row_resolution(row):
    """The finest grid of a 'pair' row's outputs: the lattice unit of its mismatch reports."""
    return min(p[2] for p in bit_budget(row))


# ---- operands ------------------------------------------------------------------------------------------------------------------
def _tern(shape, g):
    return _ints(shape, -1, 1, g, 'cpu').float()


def pair_bias(n, kind, total, g):
    """fp32 [n] bias of a 'pair' row whose largest possible |sum| is `total` (unscaled)."""
    lat = LATTICES[kind]
    if kind == 'top':
        mag = _ints((n,), TOP_BIAS[0] << TOP_BIAS_FRAC, TOP_BIAS[1] << TOP_BIAS_FRAC, g, 'cpu').float() * 2.0 ** -TOP_BIAS_FRAC
        return mag * (2 * _ints((n,), 0, 1, g, 'cpu').float() - 1)
    f = max(fine_frac(total), BIAS_FRAC)
    coarse = _ints((n,), -(E.BIAS_MAX << BIAS_FRAC), E.BIAS_MAX << BIAS_FRAC, g, 'cpu').float() * 2.0 ** -BIAS_FRAC
    fine = _ints((n,), -(E.BIAS_MAX << f), E.BIAS_MAX << f, g, 'cpu').float() * 2.0 ** -f
    return torch.where(torch.arange(n) % 2 == 1, fine, coarse) * 2.0 ** lat.scale_exp


PairOperands = collections.namedtuple('PairOperands', 'x_hi x_lo w_hi w_lo bias res_hi res_lo')


def pair_operands(row, seed=None):
    """fp32 CPU tensors, every one an fp16 number: x planes [B,H,W,Cin], w planes [Cout,k,k,Cin], bias [Cout], residual planes
    [B,OH,OW,Cout] or None.  Asserts the row's bit budget."""
    bit_budget(row)
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
    lat = LATTICES[kind]
    g = torch.Generator().manual_seed(row_seed(row) if seed is None else seed)
    OH, OW = out_hw(H, W, k, stride, pad)
    sc = 2.0 ** lat.scale_exp
    x_hi = _ints((B, H, W, Cin), 0, lat.x_max, g, 'cpu').float()
    x_lo = _tern((B, H, W, Cin), g) * 2.0 ** -XL_FRAC
    w_hi = _ints((Cout, k, k, Cin), -lat.w_max, lat.w_max, g, 'cpu').float() * sc
    w_lo = _tern((Cout, k, k, Cin), g) * 2.0 ** -lat.wl_frac * sc
    bias = pair_bias(Cout, kind, _sum_mag(k * k * Cin, lat, use_res)[1], g)
    res_hi = _ints((B, OH, OW, Cout), -E.RES_MAX, E.RES_MAX, g, 'cpu').float() if use_res else None
    res_lo = _ints((B, OH, OW, Cout), -RES_LO_MAX, RES_LO_MAX, g, 'cpu').float() * 2.0 ** -7 if use_res else None
    for t in (x_hi, x_lo, w_hi, w_lo, res_hi, res_lo):
        assert t is None or torch.equal(t.half().float(), t)
    return PairOperands(x_hi, x_lo, w_hi, w_lo, bias, res_hi, res_lo)


# ---- references ----------------------------------------------------------------------------------------------------------------
def _nchw(t, precision):
    return t.to('cpu', precision).permute(0, 3, 1, 2)


def pair_value(x_hi, x_lo, w_hi, w_lo, bias, res_hi=None, res_lo=None, stride=1, pad=0, relu=True, precision=torch.float64,
               products=('hh', 'hl', 'lh')):
    """The documented sum of NHWC / [Cout,R,S,Cin] planes on the CPU in `precision`, NHWC, BEFORE the split: the products named
    in `products` ('hh' w_hi.x_hi, 'hl' w_hi.x_lo, 'lh' w_lo.x_hi; 'll', which no kernel forms, for the CPU test's what-if),
    each its own convolution, + bias (+ res_hi (+ res_lo)), ReLU.  x_lo None: a single-plane x."""
    conv = lambda x, w: F.conv2d(_nchw(x, precision), _nchw(w, precision), None, stride, pad)      # noqa: E731
    v = None
    for name, x, w in (('hh', x_hi, w_hi), ('hl', x_lo, w_hi), ('lh', x_hi, w_lo), ('ll', x_lo, w_lo)):
        if name in products and x is not None:
            v = conv(x, w) if v is None else v + conv(x, w)
    v = v + bias.to('cpu', precision).view(1, -1, 1, 1)
    for r in (res_hi, res_lo):
        if r is not None:
            v = v + _nchw(r, precision)
    if relu:
        v = F.relu(v)
    return v.permute(0, 2, 3, 1).contiguous()


def as_fp32(v64, what=''):
    """The fp64 reference value as the fp32 number the kernel holds: on lattice operands the conversion is exact (asserted)."""
    v = v64.float()
    assert torch.equal(v.double(), v64), '%s: the fp64 reference is not an fp32 number - the operands left the lattice' % what
    return v


def split_value(v):
    """The pair output of an fp32 value: hi = RNE_fp16(v), lo = RNE_fp16(v - hi) (torch's .half() rounds to nearest even and
    keeps subnormals; v - hi is exact in fp32)."""
    assert v.dtype == torch.float32
    hi = v.half()
    return hi, (v - hi.float()).half()


def pair_reference(ops, row, x_pair=True, res_planes=2):
    """(hi, lo, fp32 value) a kernel must give on PairOperands `ops` of `row` with x as a pair or its hi plane alone and 2, 1 or
    0 residual planes."""
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
    v = as_fp32(pair_value(ops.x_hi, ops.x_lo if x_pair else None, ops.w_hi, ops.w_lo, ops.bias,
                           ops.res_hi if res_planes >= 1 else None, ops.res_lo if res_planes >= 2 else None, stride, pad, relu), tag)
    return split_value(v) + (v,)


def mismatch_pair(got, want, what, BM=128, BN=128, value=None, resolution=2.0 ** -10):
    """exact_conv.report_mismatch for both planes of a pair: fails unless got == want bit for bit in hi AND lo; the text names,
    per plane, the first differing (pixel, channel), its tile, both bit patterns and the distance from the value the plane
    should hold (hi: the fp32 value; lo: value - hi) in lattice units.  got[1] None: a single-plane output, hi alone."""
    msgs = []
    for plane, g, w, v in (('hi', got[0], want[0], value), ('lo', got[1], want[1], None if value is None else value - want[0].float())):
        if g is None:
            continue
        m = E.mismatch_report(g.cpu(), w, '%s: %s plane' % (what, plane), BM, BN, v, resolution)
        if m is not None:
            msgs.append(m)
    assert not msgs, '\n'.join(msgs)


def pair_stats(v, hi, lo):
    """Shares the CPU test asserts: (outputs that are positive, positive outputs hi alone cannot hold, positive outputs with a
    non-zero lo, non-zero outputs with hi + lo != v, non-zero outputs whose lo is an fp16 subnormal, ... whose hi is one)."""
    v, h, l = v.reshape(-1).double(), hi.reshape(-1).double(), lo.reshape(-1).double()
    pos, nz = v > 0, v != 0
    n_pos, n_nz = max(int(pos.sum()), 1), max(int(nz.sum()), 1)
    sub = lambda t: (t != 0) & (t.abs() < E.FP16_MIN_NORMAL)      # noqa: E731
    return (float(pos.sum()) / v.numel(), float((pos & (h != v)).sum()) / n_pos, float((pos & (l != 0)).sum()) / n_pos,
            float((nz & (h + l != v)).sum()) / n_nz, float((nz & sub(l)).sum()) / n_nz, float((nz & sub(h)).sum()) / n_nz)


# ---- rows ----------------------------------------------------------------------------------------------------------------------
PATCH_RAGGED = (2, 7, 45, 64, 64, 3, 1, 1, False, True)      # patch kernel: width % 32 != 0, height % 4 != 0, two images
TOP_ROW = ('top_binade_1x1_k64', 2, 9, 15, 64, 128, 1, 1, 0, False, False, 'top')
SCALED_ROW = ('scaled_1x1_k64', 2, 9, 15, 64, 64, 1, 1, 0, False, True, 'scaled')
DUAL_SHAPES = [(2, 16, 24, 64, 256), (1, 9, 13, 64, 128), (1, 7, 9, 128, 256)]      # test_pair_conv_dual_equals_downsample_plus_conv3's
SEAM_WP_SHAPES = [(2, 16, 24, 64, True), (1, 9, 13, 64, True), (1, 33, 31, 128, True), (2, 16, 16, 128, False)]   # test_seam_with_paired_weights'
# conv_c3c1ds_lc_kernel: workgroup g of min(tiles, CUs) takes the 64-pixel tiles g, g + CUs, ... - two tiles on two workgroups; 72
# tiles, the last ragged, one per workgroup; 517 tiles on the MI355X's 256 CUs: three (odd) on five workgroups, two (even) on the rest
SEAM_DS_SHAPES = [(1, 9, 13), (3, 37, 41), (3, 105, 105)]
STEM_SIZES = [(1, 7, 9), (1, 75, 61), (2, 64, 96), (1, 97, 130)]
U8_SIZES = [(1, 7, 8), (2, 8, 9), (1, 41, 53), (2, 61, 76)]


def geom_row(g, kind='std'):
    return ('%dx%dx%dx%d-%d-k%ds%d' % tuple(g[:7]) + ('-res' if g[8] else '') + ('' if g[9] else '-norelu'),) + tuple(g) + (kind,)


def conv_rows():
    """The rows of the conv_bn_act_pair tests: test_pair_gpu.GEOMS, the ragged patch row, the top-binade and the scaled row."""
    from test_pair_gpu import GEOMS
    return [geom_row(g) for g in list(GEOMS) + [PATCH_RAGGED]] + [TOP_ROW, SCALED_ROW]


def is_patch_row(row):
    """conv_pair_patch64_kernel's shapes (pair_patch64_admissible, x a pair): 3x3 stride 1 pad 1, 64 -> 64, no residual."""
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, kind = row
    return k == 3 and stride == 1 and pad == 1 and Cin == 64 and Cout == 64 and not use_res


def dual_row(shape):
    """conv_pair_dual as the paired 1x1 convolution of its concatenated K."""
    B, H, W, C, Cout = shape
    return ('pair_dual_%dx%dx%d_k%d+%d-%d' % (B, H, W, C, C, Cout), B, H, W, 2 * C, Cout, 1, 1, 0, False, True, 'std')


DualOperands = collections.namedtuple('DualOperands', 't_hi t_lo x_hi x_lo w_hi w_lo b3 bd')


def dual_operands(shape):
    """conv_pair_dual's operands: t2 and x pairs [B,H,W,C], the weight pair [Cout, 2 C] = [w3 | wds], b3 as pair_bias draws it
    for the whole sum (both biases: |b3 + bd| <= 64), bd on the 2^-7 grid so that the downsample's own output fits a pair."""
    bit_budget(shape, 'pair_dual')
    B, H, W, C, Cout = shape
    lat = LATTICES['std']
    g = torch.Generator().manual_seed(row_seed(dual_row(shape)))
    t_hi, x_hi = (_ints((B, H, W, C), 0, lat.x_max, g, 'cpu').float() for _ in range(2))
    t_lo, x_lo = (_tern((B, H, W, C), g) * 2.0 ** -XL_FRAC for _ in range(2))
    w_hi = _ints((Cout, 2 * C), -lat.w_max, lat.w_max, g, 'cpu').float()
    w_lo = _tern((Cout, 2 * C), g) * 2.0 ** -lat.wl_frac
    b3 = pair_bias(Cout, 'std', _sum_mag(2 * C, lat, False, 2 * E.BIAS_MAX)[1], g)
    bd = _ints((Cout,), -(E.BIAS_MAX << BIAS_FRAC), E.BIAS_MAX << BIAS_FRAC, g, 'cpu').float() * 2.0 ** -BIAS_FRAC
    return DualOperands(t_hi, t_lo, x_hi, x_lo, w_hi, w_lo, b3, bd)


def dual_reference(o, relu=True):
    """(hi, lo, value) of relu([w3 | wds] . [t2 ; x] + b3 + bd) with three products per term."""
    C = o.t_hi.shape[-1]
    w = lambda t, a: t[:, a * C:(a + 1) * C].reshape(t.shape[0], 1, 1, C)      # noqa: E731
    v = (pair_value(o.t_hi, o.t_lo, w(o.w_hi, 0), w(o.w_lo, 0), o.b3, relu=False) +
         pair_value(o.x_hi, o.x_lo, w(o.w_hi, 1), w(o.w_lo, 1), o.bd, relu=False))
    v = as_fp32(F.relu(v) if relu else v, 'pair_dual')
    return split_value(v) + (v,)


SeamOperands = collections.namedtuple('SeamOperands', 't2 x_hi x_lo w3_hi w3_lo b3 res w1_hi w1_lo b1')


def seam_wp_operands(shape, ds=False, seed=0):
    """Operands of conv_c3c1_wpair (ds False: w3 planes [256, 64], res [B,H,W,256], x planes None) or conv_c3c1_ds_wpair (ds True:
    x planes [B,H,W,64], w3 planes [256, 128] = [w3 | wds], res None); shape = (B, H, W, P2, w1 is a pair).  fp32 CPU tensors of
    fp16 numbers; asserts the seam's bit budget."""
    bit_budget(shape, 'seam_ds_wp' if ds else 'seam_wp')
    B, H, W, P2, w1_pair = shape
    yf, y_max, f1 = seam_wp_geometry(ds)
    g = torch.Generator().manual_seed(seed)
    t2 = _ints((B, H, W, 64), 0, E.X_MAX, g, 'cpu').float()
    x_hi = _ints((B, H, W, 64), 0, E.X_MAX, g, 'cpu').float() if ds else None
    x_lo = _tern((B, H, W, 64), g) * 2.0 ** -yf if ds else None
    K3 = 128 if ds else 64
    w3_hi = _ints((256, K3), -E.W_MAX, E.W_MAX, g, 'cpu').float()
    w3_lo = _tern((256, K3), g) * 2.0 ** -yf
    b3 = _ints((256,), -E.BIAS_MAX, E.BIAS_MAX, g, 'cpu').float()
    res = None if ds else _ints((B, H, W, 256), -E.RES_MAX, E.RES_MAX, g, 'cpu').float()
    rw = 2.0 ** -f1
    w1_hi = _ints((P2, 256), -E.W_MAX, E.W_MAX, g, 'cpu').float() * rw
    w1_lo = _tern((P2, 256), g) * (rw / 8)
    b1 = E.lattice_bias(P2, y_max * (E.W_MAX * rw + rw / 8) * 256 + E.BIAS_MAX, g, 'cpu')
    return SeamOperands(t2, x_hi, x_lo, w3_hi, w3_lo, b3, res, w1_hi, w1_lo if w1_pair else None, b1)


def seam_wp_reference(o, relu3=True, relu1=True):
    """(y, t1, y's value, t1's value): y = RNE_fp16(act3(...)) as the module docstring states it, t1 from the ROUNDED y, fp64."""
    d = lambda t: t.double()      # noqa: E731
    B, H, W, _ = o.t2.shape
    t2 = d(o.t2).reshape(-1, 64)
    w3 = d(o.w3_hi) + d(o.w3_lo)
    vy = t2 @ w3[:, :64].T + d(o.b3)
    if o.x_hi is not None:
        vy = vy + d(o.x_hi).reshape(-1, 64) @ w3[:, 64:].T + d(o.x_lo).reshape(-1, 64) @ d(o.w3_hi)[:, 64:].T
    if o.res is not None:
        vy = vy + d(o.res).reshape(-1, 256)
    vy = as_fp32(F.relu(vy) if relu3 else vy, 'seam y')
    y = vy.half()
    w1 = d(o.w1_hi) + (d(o.w1_lo) if o.w1_lo is not None else 0)
    vt = d(y) @ w1.T + d(o.b1)
    vt = as_fp32(F.relu(vt) if relu1 else vt, 'seam t1')
    return y.reshape(B, H, W, 256), vt.half().reshape(B, H, W, -1), vy.reshape(B, H, W, 256), vt.reshape(B, H, W, -1)


# ---- the paired stem ---------------------------------------------------------------------------------------------------------
def stem_row(bhw):
    B, H, W = bhw
    return ('stem_pair_%dx%dx%d' % bhw, B, H, W, 3, 64, 7, 2, 3, False, True, 'stem')


def s2d(img_nchw):
    """[B,3,H,W] -> the 2x2 space-to-depth form [B,(H+1)/2,(W+1)/2,16] the stem kernels read: channel (dy 2 + dx) 3 + c, zeros in
    channels 12 ... 15 and past an odd edge."""
    B, C, H, W = img_nchw.shape
    out = torch.zeros(B, (H + 1) // 2, (W + 1) // 2, 16, dtype=img_nchw.dtype)
    for dy in range(2):
        for dx in range(2):
            sub = img_nchw[:, :, dy::2, dx::2].permute(0, 2, 3, 1)
            out[:, :sub.shape[1], :sub.shape[2], (dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3] = sub
    return out


StemOperands = collections.namedtuple('StemOperands', 'x_hi x_lo w w_hi w_lo bias')


def stem_operands(bhw):
    """A lattice image pair (NCHW planes) and a lattice 7x7 filter: w [64,3,7,7] fp32 = a + s 2^-12, whose split_pair is exactly
    (w_hi, w_lo) = (a, s 2^-12) (asserted)."""
    row = stem_row(bhw)
    bit_budget(row)
    B, H, W = bhw
    lat = LATTICES['stem']
    g = torch.Generator().manual_seed(row_seed(row))
    x_hi = _ints((B, 3, H, W), 0, lat.x_max, g, 'cpu').float()
    x_lo = _tern((B, 3, H, W), g) * 2.0 ** -XL_FRAC
    w_hi = _ints((64, 3, 7, 7), -lat.w_max, lat.w_max, g, 'cpu').float()
    w_lo = torch.where(w_hi != 0, _tern((64, 3, 7, 7), g), torch.zeros(())) * 2.0 ** -lat.wl_frac
    w = w_hi + w_lo
    hi = w.half()
    assert torch.equal(hi.float(), w_hi) and torch.equal((w - hi.float()).half().float(), w_lo)
    bias = pair_bias(64, 'stem', _sum_mag(147, lat, False)[1], g)
    return StemOperands(x_hi, x_lo, w, w_hi, w_lo, bias)


def stem_reference(o):
    """(hi, lo, value) [B,PH,PW,64] of split(maxpool3x3s2(relu(conv7x7s2 + bias))) in fp64."""
    nhwc = lambda t: t.permute(0, 2, 3, 1)      # noqa: E731
    v = pair_value(nhwc(o.x_hi), nhwc(o.x_lo), nhwc(o.w_hi), nhwc(o.w_lo), o.bias, None, None, 2, 3, True)
    v = F.max_pool2d(v.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    v = as_fp32(v, 'paired stem')
    return split_value(v) + (v,)


# ---- the stem on the raw uint8 image (csrc/stem_u8.hip) --------------------------------------------------------------------------
# fold_stem_u8 (host, double) turns ToTensor + Normalize + conv + BatchNorm into w' = w scale 256 / (255 std_c) as an fp16 pair, the
# bias b2 = bias - sum_{147 taps} w scale mean_c / std_c and a border table of the taps that fall outside the image; the kernel forms
# max-pool(sum_{all taps} w' (u / 256) + border term) + b2, ReLU.  Every step is exact when w = 255 t 2^-k (then w' = t' 2^-6, t' =
# 64 a + s, a and s in {-1, 0, 1}), std and scale are powers of two and mean is 1/2 or 1: a folded term w' 255 mean / 256 is a
# multiple of 2^-15, and so are the bias, the border term and the output.  What cannot be had together with that is a NON-ZERO lo
# plane of w': a tap of more than 11 bits makes 255 mean w' a 20-bit number and the 147-term bias a 28-bit one, which the fold's own
# (float)(bias - sum) rounds.  So here w'_lo = 0 (asserted): these cases check the hi product, the fold, the border classes, the
# pooling in registers and the output split, at both planes of the output.
U8_MEAN, U8_STD = (0.5, 1.0, 0.5), (0.25, 0.5, 0.25)
U8_W_FRAC = 6            # w' = a + s 2^-6


def u8_budget():
    """bit_budget of the uint8 stem (the same at every size): the kernel's sum over all 147 taps, + the border term, + the
    folded bias; every operand and the result a multiple of 2^-15."""
    wmax = 1 + 2.0 ** -U8_W_FRAC
    s_all = 147 * wmax * 255 / 256                  # sum w' u / 256 on the 2^-14 grid
    fold = 147 * wmax * max(U8_MEAN) * 255 / 256    # |sum w' 255 mean / 256|, and every part of it (the border table)
    return _audit([('all 147 taps of w\' . u / 256', s_all, 2.0 ** -(U8_W_FRAC + 8)),
                   ('+ the border term', s_all + fold, 2.0 ** -15),
                   ('the folded bias b2', E.BIAS_MAX + fold, 2.0 ** -15),
                   ('output: taps inside the image + bias', 147 * wmax * 255 / 256 + E.BIAS_MAX, 2.0 ** -15)])


U8Operands = collections.namedtuple('U8Operands', 'img w scale bias w_folded')


def u8_operands(bhw):
    """A random uint8 NHWC image, conv1.weight [64,3,7,7] = 255 t 2^-k, the folded BatchNorm scale (a power of two per channel)
    and bias, and the folded filter w' the kernel must end up with (fp32, [64,3,7,7])."""
    u8_budget()
    B, H, W = bhw
    g = torch.Generator().manual_seed(row_seed(('stem_u8_%dx%dx%d' % bhw,)))
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    wf = _ints((64, 3, 7, 7), -1, 1, g, 'cpu').float() + _tern((64, 3, 7, 7), g) * 2.0 ** -U8_W_FRAC
    scale = 2.0 ** (torch.arange(64) % 3 - 1).float()
    std = torch.tensor(U8_STD).view(1, 3, 1, 1)
    w = wf * 255 * std / (256 * scale.view(64, 1, 1, 1))
    assert torch.equal(w.double(), wf.double() * 255 * std.double() / (256 * scale.double().view(64, 1, 1, 1)))      # exact in fp32
    coarse = _ints((64,), -(E.BIAS_MAX << 7), E.BIAS_MAX << 7, g, 'cpu').float() * 2.0 ** -7
    fine = _ints((64,), -(E.BIAS_MAX << 15), E.BIAS_MAX << 15, g, 'cpu').float() * 2.0 ** -15
    return U8Operands(img, w, scale, torch.where(torch.arange(64) % 2 == 1, fine, coarse), wf)


def u8_fold(o):
    """fold_stem_u8's arithmetic, step by step in fp64 as the host code does it, with every rounding to fp32 ASSERTED to be exact:
    returns (w' as fp32 [64,3,7,7], b2 [64] fp32)."""
    w, sc = o.w.double(), o.scale.double().view(64, 1, 1, 1)
    mean, std = torch.tensor(U8_MEAN).double().view(1, 3, 1, 1), torch.tensor(U8_STD).double().view(1, 3, 1, 1)
    ws = w * sc
    wp = ws * 256.0 / (255.0 * std)
    assert torch.equal(wp.float().double(), wp) and torch.equal(wp.float(), o.w_folded), 'the folded filter is not exact'
    hi = wp.float().half()
    assert torch.equal(hi.float(), o.w_folded), 'the folded filter has a lo plane'
    terms = ws * (mean / std)
    assert torch.equal(terms, o.w_folded.double() * 255 * mean / 256), 'a folded bias term is not exact'
    b2 = o.bias.double() - terms.sum((1, 2, 3))
    assert torch.equal(b2.float().double(), b2), 'the folded bias is not an fp32 number'
    # the border table: every partial sum of `terms` over a sub-rectangle of taps - multiples of 2^-15 below 2^9 (u8_budget)
    assert torch.equal((terms * 2.0 ** 15).round(), terms * 2.0 ** 15)
    return wp.float(), b2.float()


def u8_reference(o):
    """(hi, lo, value) of the reference's own definition - ToTensor, Normalize, zero padding, conv 7x7 s2, BN, ReLU, max-pool 3x3
    s2 - in fp64 with the one inexact step (u / 255) multiplied through: w ((u / 255 - mean) / std) scale = w'' (u - 255 mean),
    w'' = w scale / (255 std) exact for these operands.  The literal chain in fp64 agrees to fp64's own rounding (asserted)."""
    mean, std = torch.tensor(U8_MEAN).double().view(1, 3, 1, 1), torch.tensor(U8_STD).double().view(1, 3, 1, 1)
    u = o.img.permute(0, 3, 1, 2).double()
    w2 = o.w.double() * o.scale.double().view(64, 1, 1, 1) / (255.0 * std)
    assert torch.equal(w2 * 256, o.w_folded.double())
    v = F.conv2d(u - 255.0 * mean, w2, o.bias.double(), 2, 3)
    literal = F.conv2d((u / 255.0 - mean) / std, o.w.double(), None, 2, 3) * o.scale.double().view(1, 64, 1, 1) + o.bias.double().view(1, 64, 1, 1)
    assert float((literal - v).abs().max()) < 1e-9
    v = F.max_pool2d(F.relu(v), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    v = as_fp32(v, 'uint8 stem')
    return split_value(v) + (v,)

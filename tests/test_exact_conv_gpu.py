"""Every 16-bit convolution kernel, and the strict fp32 one, BIT FOR BIT against the CPU on operands whose fp32 sums are exact in
every order (tests/exact_conv.py: the lattice, its bit budget and the reference; tests/test_exact_lattice_cpu.py checks on the
CPU that the reference is exact and that rounding, ties and the ReLU are exercised on every row used here).

The tolerance tests (test_ops_gpu.py and its kin) keep realistic magnitudes and find index bugs; they accept four times a
correct store's rounding error, so arithmetic that is subtly wrong - a pack that truncates, a partial sum that passes through
16 bits, a bias or residual added after the rounding - passes that gate (three such mutants of conv_igemm.hip were caught by
the old suite only where it compares two kernels with each other, never by the tolerance; every one fails here in hundreds of
cases).  Here the only rounding is the store, so

    got == RNE_dtype(act(exact_sum + bias + res))      with zero tolerance,

for every admissible (CONV_SHAPES row, variant) pair, the naive kernel, split-K in every factor on every variant that splits,
the fused seam (with and without the downsample as extra K), the two-source GEMM in its three kernels, the fused stem + pool in
both forms, and dir_conv_bn_act_f32.  A failure names the first differing (m, n), its tile, both bit patterns and the
distance from the fp32 value in lattice units.

The first test anchors the device itself: the naive kernel (plain FMAs) and one MFMA tile kernel on one small row.  Were the
MFMA alone to disagree there, v_mfma_f32_32x32x16_{bf16,f16} would not add these terms without loss and the lattice would have to
shrink.  On the MI355X both reproduce the CPU's bits in bf16 and in fp16, and so does every other kernel below.

The paired-fp16 entry points (conv_bn_act_pair, conv_pair_dual, conv_c3c1_wpair, conv_c3c1_ds_wpair, the paired stems) have a
lattice with lo planes and a budget of its own: tests/exact_pair.py, compared bit for bit in both planes by
tests/test_exact_pair_gpu.py.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_conv as E
from test_ops_gpu import CONV_CASES, SPLITK_SHAPES

pytestmark = pytest.mark.gpu

DNAMES = ('bf16', 'fp16')


def _ops():
    from dirtorch_amd import ops
    return ops


def _tile(vname):
    return tuple(int(v) for v in vname.split('_')[0].split('x'))


@functools.lru_cache(maxsize=2)      # (cases run row by row: one row's operands and reference at a time)
def _plain(row):
    """fp32 copies of the row's lattice operands (exact in both 16-bit formats) and the fp32 value before the store."""
    x, w, bias, res = E.lattice_operands(row, torch.float32)
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = row
    return x, w, bias, res, E.exact_value(x, w, bias, res, stride, pad, relu)


def _device_args(row, dt):
    x, w, bias, res, value = _plain(row)
    return (x.to(dt).cuda(), w.to(dt).cuda(), bias.cuda(), None if res is None else res.to(dt).cuda()), value


def _check(y, value, dt, what, BM=64, BN=64):
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(value.shape), (y.shape, value.shape)
    E.report_mismatch(y.cpu(), value.to(dt), what, BM, BN, value)


@pytest.mark.parametrize('dname', DNAMES)
def test_anchor_naive_and_one_mfma_tile(dname):
    """The plain-FMA kernel and the 128x128_w2x2 MFMA tile on one small row, both bitwise against the CPU."""
    ops = _ops()
    row, dt = E.ANCHOR_ROW, E.DTYPES[dname]
    args, value = _device_args(row, dt)
    kw = dict(stride=row[7], pad=row[8], relu=row[10])
    _check(ops.conv_bn_act(*args, naive=True, **kw), value, dt, 'anchor: naive kernel ' + dname)
    _check(ops.conv_bn_act(*args, variant=ops.conv_variant_names().index('128x128_w2x2'), **kw), value, dt,
           'anchor: 128x128_w2x2 ' + dname, 128, 128)


VARIANT_CASES = [(s, v, d) for s, v in CONV_CASES for d in DNAMES]


@pytest.mark.parametrize('shape,vname,dname', VARIANT_CASES, ids=['%s-%s-%s' % (s[0], v, d) for s, v, d in VARIANT_CASES])
def test_conv_variant_bitwise(shape, vname, dname):
    ops = _ops()
    dt = E.DTYPES[dname]
    args, value = _device_args(shape, dt)
    y = ops.conv_bn_act(*args, stride=shape[7], pad=shape[8], relu=shape[10], variant=ops.conv_variant_names().index(vname))
    _check(y, value, dt, '%s variant %s %s' % (shape[0], vname, dname), *_tile(vname))


@pytest.mark.parametrize('dname', DNAMES)
def test_naive_conv_bitwise(dname):
    ops = _ops()
    row, dt = E.NAIVE_ROW, E.DTYPES[dname]
    args, value = _device_args(row, dt)
    _check(ops.conv_bn_act(*args, stride=row[7], pad=row[8], relu=row[10], naive=True), value, dt, 'naive conv ' + dname)


def _split_variants():
    """The variants that have a split-K form: those the library gives more than one slice on a long-K shape of a few tiles."""
    try:
        names = _ops().conv_variant_names()
    except Exception:
        return []
    probe = (1, 5, 5, 2048, 512, 1, 1, 0, False)
    return [n for v, n in enumerate(names) if E.variant_admissible(v, probe) and E.variant_splitk(v, probe) > 1]


SPLIT_CASES = [(s, v, k, d) for s in SPLITK_SHAPES for v in _split_variants() for k in (2, 3, 4, 8, -1) for d in DNAMES]


def test_split_variants_are_the_four_igemm_tiles_with_a_split_form():
    assert _split_variants() == ['128x128_w2x2', '64x128_w2x2', '64x64_w2x2_s8', '64x64_w2x2_s4']


@pytest.mark.parametrize('shape,vname,ksplit,dname', SPLIT_CASES, ids=['%s-%s-k%d-%s' % (s[0], v, k, d) for s, v, k, d in SPLIT_CASES])
def test_conv_splitk_bitwise(shape, vname, ksplit, dname):
    """K cut into 2, 3, 4, 8 slices and into the engine's own number: the slices' fp32 partial sums and their sum are exact, so
    every factor gives the unsplit result bit for bit."""
    ops = _ops()
    dt = E.DTYPES[dname]
    args, value = _device_args(shape, dt)
    y = ops.conv_bn_act(*args, stride=shape[7], pad=shape[8], relu=shape[10], variant=ops.conv_variant_names().index(vname), ksplit=ksplit)
    used = ops.conv_bn_act.last_ksplit
    assert used == ksplit if ksplit > 0 else used >= 2, used      # these shapes all split when the engine chooses
    _check(y, value, dt, '%s %s split-K %d %s' % (shape[0], vname, used, dname), *_tile(vname))


SEAM_CASES = [(c, r, d) for c in E.seam_cases() for r in (True, False) for d in DNAMES if not (c[5] and not r)]


@pytest.mark.parametrize('case,relu3,dname', SEAM_CASES,
                         ids=['%dx%dx%d-P%d-P%d-%s-%s-%s' % (c[:5] + ('ds' if c[5] else 'res', 'relu' if r else 'norelu', d)) for c, r, d in SEAM_CASES])
def test_fused_seam_bitwise(case, relu3, dname):
    """conv_c3c1 / conv_c3c1_ds: y = RNE(act3(conv3 + b3 + res)) and t1 = RNE(relu(RNE(y) . w1 + b1)), both bit for bit (the
    reference rounds y exactly where the kernel does)."""
    ops = _ops()
    B, H, W, P, P2, ds = case
    dt = E.DTYPES[dname]
    t2, w3, b3, other, w1, b1 = E.seam_operands((B, H, W, P, P2), dt, seed=E.zlib.crc32(repr(case).encode()), ds=ds)
    dev = [t.cuda() for t in (t2, w3, b3, other, w1, b1)]
    if ds:
        y, t1 = ops.conv_c3c1_ds(dev[0], dev[3], dev[1], dev[2], dev[4], dev[5], relu3=relu3, relu1=True)
        want_y, want_t1, vy, vt = E.seam_reference(t2, w3, b3, None, w1, b1, relu3, True, dt, x=other)
    else:
        y, t1 = ops.conv_c3c1(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], relu3=relu3, relu1=True)
        want_y, want_t1, vy, vt = E.seam_reference(t2, w3, b3, other, w1, b1, relu3, True, dt)
    torch.cuda.synchronize()
    what = 'seam %r relu3 %d %s' % (case, relu3, dname)
    E.report_mismatch(y.cpu(), want_y, what + ': block output y', 64, 4 * P, vy, 1.0)
    E.report_mismatch(t1.cpu(), want_t1, what + ': next conv1 t1', 64, P2, vt)


DUAL_CASES = [(s, d) for s in E.dual_shapes() for d in DNAMES]


@pytest.mark.parametrize('shape,dname', DUAL_CASES, ids=['%dx%dx%d-%d-%d-%d-s%d-%s' % (s + (d,)) for s, d in DUAL_CASES])
def test_two_source_gemm_bitwise(shape, dname, monkeypatch):
    """conv_dual: act([w3 | wds] . [t2 ; x strided] + bias) in the kernel the library picks (conv_wregd.hip on layer2's K = 128 +
    256), in the generic two-source ring (conv_persist.hip) and in its loader / consumer form (conv_persistlc.hip): with exact
    sums the three agree with the CPU - and so with each other - bit for bit, wherever each adds the bias."""
    ops = _ops()
    B, OH, OW, Cin, Cout, Cin2, s2 = shape
    dt = E.DTYPES[dname]
    row = E.dual_row(shape)
    E.bit_budget(row)
    g = torch.Generator().manual_seed(E.row_seed(row))
    H2, W2 = (OH - 1) * s2 + 1 + (s2 - 1), (OW - 1) * s2 + 1
    t2 = E._ints((B, OH, OW, Cin), 0, E.X_MAX, g, 'cpu').float()
    x = E._ints((B, H2, W2, Cin2), 0, E.X_MAX, g, 'cpu').float()
    wcat = E.lattice_weights((Cout, Cin + Cin2), g, 'cpu')
    bias = E.lattice_bias(Cout, E.X_MAX * E.W_MAX * (Cin + Cin2) + E.BIAS_MAX, g, 'cpu')
    value = (E.exact_value(t2, wcat[:, :Cin].reshape(Cout, 1, 1, Cin), bias, None, 1, 0, False) +
             E.exact_value(x, wcat[:, Cin:].reshape(Cout, 1, 1, Cin2), torch.zeros(Cout), None, s2, 0, False))
    value = F.relu(value)
    assert value.shape[1:3] == (OH, OW)
    args = (t2.to(dt).cuda(), x.to(dt).cuda(), wcat.to(dt).cuda(), bias.cuda())
    what = 'two-source %r %s' % (shape, dname)
    _check(ops.conv_dual(*args, stride2=s2, relu=True), value, dt, what + ': the picked kernel', 64, 256)
    monkeypatch.setenv('DIRTORCH_AMD_NO_WREGD', '1')
    _check(ops.conv_dual(*args, stride2=s2, relu=True), value, dt, what + ': the generic ring', 256, 256)
    if Cout % 256 == 0 and OW > 1:
        monkeypatch.setenv('DIRTORCH_AMD_LC1X1', '1')
        _check(ops.conv_dual(*args, stride2=s2, relu=True), value, dt, what + ': the loader / consumer ring', 256, 256)


STEM_CASES = [(hw, f, d) for hw in E.STEM_SIZES for f in ('persistent', 'one_tile_per_workgroup') for d in DNAMES]


@pytest.mark.parametrize('hw,form,dname', STEM_CASES, ids=['%dx%d-%s-%s' % (hw + (f, d)) for hw, f, d in STEM_CASES])
def test_fused_stem_pool_bitwise(hw, form, dname, monkeypatch):
    """A lattice image through prep_input's fp32 feed (no normalisation), 7 x 7 lattice taps through pack_stem_weight, then
    stem_pool: == maxpool(RNE(relu(conv + bias))) bit for bit (max commutes with rounding), in both forms of the kernel."""
    if form != 'persistent':
        monkeypatch.setenv('DIRTORCH_AMD_STEM_V1', '1')
    ops = _ops()
    dt = E.DTYPES[dname]
    row = E.stem_row(hw)
    x, w, bias, _, value = _plain(row)            # NHWC image [2, H, W, 3], taps [64, 7, 7, 3]
    H, W = hw
    OH, OW = E.out_hw(H, W, 7, 2, 3)
    want = F.max_pool2d(value.to(dt).float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(dt)
    s2d = ops.prep_input(x.permute(0, 3, 1, 2).contiguous().cuda(), dt)
    wp = ops.pack_stem_weight(w.permute(0, 3, 1, 2).contiguous(), dt).cuda()
    y = ops.stem_pool(s2d, wp, bias.cuda(), (OH, OW))
    torch.cuda.synchronize()
    assert y.shape == want.shape
    E.report_mismatch(y.cpu(), want, 'stem_pool %dx%d %s %s' % (H, W, form, dname), 64, 64)
    # ... and the unfused stem convolution, whose every output is visible
    conv = ops.conv_bn_act(s2d, wp, bias.cuda(), None, stride=1, pad=2, relu=True, out_hw=(OH, OW))
    _check(conv, value, dt, 'stem conv %dx%d %s' % (H, W, dname))


F32_ROWS = E.f32_rows()


@pytest.mark.parametrize('row', F32_ROWS, ids=[r[0] for r in F32_ROWS])
def test_conv_f32_bitwise(row):
    """dir_conv_bn_act_f32 (fp32 storage, fp32 MFMA): with exact sums its fp32 output IS the CPU's fp32 convolution."""
    ops = _ops()
    x, w, bias, res, value = _plain(row)
    y = ops.conv_bn_act_f32(x.cuda(), w.cuda(), bias.cuda(), None if res is None else res.cuda(), stride=row[7], pad=row[8],
                            relu=row[10])
    _check(y, value, torch.float32, 'conv_f32 ' + row[0], 128, 128)

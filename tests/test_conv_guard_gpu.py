"""No conv kernel stores outside its output: every 16-bit conv entry point, called through the C ABI with each output plane in
the MIDDLE of a larger buffer, leaves 4096 elements of a fixed bit pattern on both sides of the plane untouched and fills the
plane with the very bits the ordinary ops wrapper returns for the same operands.

The exact suites (test_exact_conv_gpu.py, test_exact_pair_gpu.py) and the tolerance suites compare the output tensor; a store
that lands past it - a dropped `m < M` on the ragged last pixel tile, an `ox < OW` that became `<=` - leaves that tensor right
and goes unseen.  The store masks are what a change to an epilogue transcribes, kernel by kernel; the rows here are the ragged
ones of test_ops_gpu.CONV_SHAPES (126, 442, 1334 pixels; 13 x 37, 37 x 33, 19 x 35, 9 x 17 maps) on every admissible variant.

The guards are a multiple of 8 elements, so the planes keep the 16-byte alignment the entry points ask for.  The planes start
out filled with the pattern as well: an element the kernel never wrote differs from the wrapper's result.  Nothing here is
compared with a tolerance.

The 592 (row, variant) pairs x 2 dtypes of dir_conv_bn_act are ONE pytest case per (row, dtype): the row's operands are made
once, every admissible variant runs on them whatever the others did, and a failure lists each variant that went wrong.  The
suite's case count stays small that way (67 cases here, under two seconds) and nothing is checked less."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import exact_conv as E
from test_ops_gpu import CONV_CASES, CONV_SHAPES, DTYPES, SPLITK_SHAPES, _rand, variant_admissible

pytestmark = pytest.mark.gpu

GUARD = 4096           # elements on each side of a plane
PATTERN = 0x5AA5       # never a value these operands produce in a whole plane; as int16: 23205


def _ops():
    from dirtorch_amd import ops
    return ops


class Guarded:
    """A 16-bit (or, words = 2, 32-bit) plane of `shape` between two guard bands, all of it pre-filled with PATTERN."""

    def __init__(self, shape, dtype, words=1):
        n = 1
        for s in shape:
            n *= s
        self.n = n * words
        self.buf = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int16, device='cuda')
        self.plane = self.buf[GUARD:GUARD + self.n].view(dtype).view(*shape)
        assert self.plane.data_ptr() % 16 == 0 and self.plane.data_ptr() == self.buf.data_ptr() + 2 * GUARD

    def check(self, want, what):
        """Guards intact, plane == want bit for bit (want None: the guards only)."""
        torch.cuda.synchronize()
        for side, band in (('below', self.buf[:GUARD]), ('above', self.buf[GUARD + self.n:])):
            hit = (band != PATTERN).nonzero().flatten()
            assert hit.numel() == 0, '%s: %d guard elements %s the plane overwritten, first at offset %d' % (
                what, hit.numel(), side, int(hit[0]) - (GUARD if side == 'below' else 0))
        if want is not None:
            got = self.plane.contiguous().view(torch.int16).flatten()
            ref = want.contiguous().view(torch.int16).flatten()
            assert got.numel() == ref.numel(), what
            bad = (got != ref).nonzero().flatten()
            assert bad.numel() == 0, '%s: %d of %d elements differ from the wrapper\'s, first at flat index %d' % (
                what, bad.numel(), got.numel(), int(bad[0]))


def _operands(shape, dt):
    name, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    OH, OW = E.out_hw(H, W, k, stride, pad)
    x = _rand((B, H, W, Cin), 1).to(dt).cuda()
    w = _rand((Cout, k, k, Cin), 2, (2.0 / (k * k * Cin)) ** 0.5).to(dt).cuda()
    bias = _rand((Cout,), 3, 0.2).cuda()
    res = _rand((B, OH, OW, Cout), 4).to(dt).cuda() if use_res else None
    return x, w, bias, res, OH, OW


def _conv_args(shape, x, w, bias, res, y, OH, OW):
    from dirtorch_amd._lib import ptr
    name, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    return [ptr(x), ptr(w), ptr(bias), ptr(res), ptr(y), B, H, W, Cin, Cout, k, k, stride, pad, OH, OW, int(bool(relu)),
            _ops()._dtype_code(x)]


def _run_plain(shape, vnames, dname):
    """One row on each of `vnames`, every variant run whatever the others did; fails with the list of those that went wrong."""
    from dirtorch_amd._lib import call, stream_ptr
    ops = _ops()
    dt = DTYPES[dname]
    names = ops.conv_variant_names()
    x, w, bias, res, OH, OW = _operands(shape, dt)
    assert vnames, 'no admissible variant for ' + shape[0]
    wrong = []
    for vname in vnames:
        variant = names.index(vname)
        want = ops.conv_bn_act(x, w, bias, res, stride=shape[7], pad=shape[8], relu=shape[10], variant=variant)
        g = Guarded((shape[1], OH, OW, shape[5]), dt)
        call('dir_conv_bn_act', *_conv_args(shape, x, w, bias, res, g.plane, OH, OW), variant, stream_ptr())
        try:
            g.check(want, '%s variant %s %s' % (shape[0], vname, dname))
        except AssertionError as e:
            wrong.append(str(e))
    assert not wrong, '%d of %d variants:\n%s' % (len(wrong), len(vnames), '\n'.join(wrong))


# one case per (row, dtype): the row's operands are made once and every admissible variant of test_ops_gpu.CONV_CASES runs on them
ROW_VARIANTS = [(s, [v for r, v in CONV_CASES if r is s]) for s in CONV_SHAPES]


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('shape,vnames', ROW_VARIANTS, ids=[s[0] for s, _ in ROW_VARIANTS])
def test_conv_variants_stay_inside_their_output(shape, vnames, dname):
    _run_plain(shape, vnames, dname)


RING_ROWS = [s for s in CONV_SHAPES if variant_admissible('128x256_ring1x1', s[4], s[5], s[6], s[7], s[8], s[9])]


@pytest.mark.experiments      # conv_ring.hip ships in experiments builds only (DIR_EXPERIMENTS=1 csrc/build.sh)
@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('shape', RING_ROWS, ids=[s[0] for s in RING_ROWS])
def test_ring_kernel_stays_inside_its_output(shape, dname):
    _run_plain(shape, ['128x256_ring1x1'], dname)


def _split_variants():
    """The variants with a split-K form (test_exact_conv_gpu.py pins their names)."""
    try:
        names = _ops().conv_variant_names()
    except Exception:
        return []
    probe = (1, 5, 5, 2048, 512, 1, 1, 0, False)
    return [n for v, n in enumerate(names) if E.variant_admissible(v, probe) and E.variant_splitk(v, probe) > 1]


SPLIT_ROW = [s for s in SPLITK_SHAPES if s[0] == '3x3_s2_res'][0]      # 112 pixels (ragged in every tile size), residual, stride 2


@pytest.mark.parametrize('dname', list(DTYPES))
@pytest.mark.parametrize('vname', _split_variants())
def test_splitk_stays_inside_its_output_and_its_partials(vname, dname):
    """Three K slices: the finalize kernel's output plane and the fp32 partial sums the conv kernel writes, both between guards."""
    from dirtorch_amd._lib import call, ptr, stream_ptr
    ops = _ops()
    shape, dt, ksplit = SPLIT_ROW, DTYPES[dname], 3
    variant = ops.conv_variant_names().index(vname)
    x, w, bias, res, OH, OW = _operands(shape, dt)
    want = ops.conv_bn_act(x, w, bias, res, stride=shape[7], pad=shape[8], relu=shape[10], variant=variant, ksplit=ksplit)
    assert ops.conv_bn_act.last_ksplit == ksplit
    g = Guarded((shape[1], OH, OW, shape[5]), dt)
    part = Guarded((ksplit, shape[1] * OH * OW, shape[5]), torch.float32, words=2)
    used = ctypes.c_int()
    call('dir_conv_bn_act_splitk', *_conv_args(shape, x, w, bias, res, g.plane, OH, OW), variant, ksplit, ptr(part.plane),
         part.plane.numel() * 4, ctypes.byref(used), stream_ptr())
    assert used.value == ksplit
    g.check(want, '%s %s split-K %d %s' % (shape[0], vname, ksplit, dname))
    part.check(None, '%s %s split-K %d %s: partial sums' % (shape[0], vname, ksplit, dname))


# the paired-fp16 conv on a ragged 3x3 row and a ragged 1x1 row, as they stand in CONV_SHAPES (3x3_patch64_ragged carries a
# residual, which only the implicit-GEMM pair kernel takes) and, so that conv_pair_patch64_kernel itself runs, the 3x3 row
# without its residual; each by default and with DIRTORCH_AMD_NO_PAIR_PATCH=1
PAIR_ROWS = [s for s in CONV_SHAPES if s[0] in ('3x3_patch64_ragged', '1x1_tail')]
PAIR_CASES = [(s, s[9]) for s in PAIR_ROWS] + [(s, False) for s in PAIR_ROWS if s[9]]


@pytest.mark.parametrize('no_patch', [False, True], ids=['default', 'NO_PAIR_PATCH'])
@pytest.mark.parametrize('shape,use_res', PAIR_CASES, ids=['%s%s' % (s[0], '' if r == s[9] else '-nores') for s, r in PAIR_CASES])
def test_paired_conv_stays_inside_both_planes(shape, use_res, no_patch, monkeypatch):
    from dirtorch_amd._lib import call, ptr, stream_ptr
    ops = _ops()
    if no_patch:
        monkeypatch.setenv('DIRTORCH_AMD_NO_PAIR_PATCH', '1')      # (the conftest wrapper calls reload_env())
    name, B, H, W, Cin, Cout, k, stride, pad, _, relu = shape
    OH, OW = E.out_hw(H, W, k, stride, pad)
    x = ops.split_pair(_rand((B, H, W, Cin), 1).cuda())
    w = ops.split_pair(_rand((Cout, k, k, Cin), 2, (2.0 / (k * k * Cin)) ** 0.5).cuda())
    bias = _rand((Cout,), 3, 0.2).cuda()
    res = ops.split_pair(_rand((B, OH, OW, Cout), 4).cuda()) if use_res else (None, None)
    want_hi, want_lo = ops.conv_bn_act_pair(x, w, bias, res if use_res else None, stride=stride, pad=pad, relu=relu)
    hi, lo = Guarded((B, OH, OW, Cout), torch.float16), Guarded((B, OH, OW, Cout), torch.float16)
    call('dir_conv_bn_act_pair', ptr(x[0]), ptr(x[1]), ptr(w[0]), ptr(w[1]), ptr(bias), ptr(res[0]), ptr(res[1]),
         ptr(hi.plane), ptr(lo.plane), B, H, W, Cin, Cout, k, k, stride, pad, OH, OW, int(bool(relu)), stream_ptr())
    what = 'pair %s%s%s' % (name, '' if use_res else ' without residual', ' NO_PAIR_PATCH' if no_patch else '')
    hi.check(want_hi, what + ': hi plane')
    lo.check(want_lo, what + ': lo plane')


def _seam_operands(B, H, W, P, P2, dt):
    t2 = F.relu(_rand((B, H, W, P), 1)).to(dt).cuda()
    w3 = _rand((4 * P, P), 2, (2.0 / P) ** 0.5)
    b3 = _rand((4 * P,), 3, 0.2).cuda()
    res = F.relu(_rand((B, H, W, 4 * P), 4)).to(dt).cuda()
    w1 = _rand((P2, 4 * P), 5, (2.0 / (4 * P)) ** 0.5)
    b1 = _rand((P2,), 6, 0.2).cuda()
    return t2, w3, b3, res, w1, b1


SEAM = (2, 9, 7, 64, 64)      # 126 pixels: one whole 64-pixel tile and a ragged one


@pytest.mark.parametrize('dname', list(DTYPES))
def test_fused_seam_stays_inside_y_and_t1(dname):
    from dirtorch_amd._lib import call, ptr, stream_ptr
    ops = _ops()
    B, H, W, P, P2 = SEAM
    dt = DTYPES[dname]
    t2, w3, b3, res, w1, b1 = _seam_operands(B, H, W, P, P2, dt)
    w3, w1 = w3.to(dt).cuda(), w1.to(dt).cuda()
    want_y, want_t1 = ops.conv_c3c1_keep(t2, w3, b3, res, w1, b1)
    y, t1 = Guarded((B, H, W, 4 * P), dt), Guarded((B, H, W, P2), dt)
    call('dir_conv_c3c1_keep', ptr(t2), ptr(w3), ptr(b3), ptr(res), ptr(y.plane), ptr(w1), ptr(b1), ptr(t1.plane), B, H, W, P, P2,
         1, 1, 0, ops._dtype_code(t2), stream_ptr())
    y.check(want_y, 'conv_c3c1_keep %s: y' % dname)
    t1.check(want_t1, 'conv_c3c1_keep %s: t1' % dname)


def test_fused_seam_with_paired_weights_stays_inside_y_and_t1():
    from dirtorch_amd._lib import call, ptr, stream_ptr
    ops = _ops()
    B, H, W, P, P2 = SEAM
    t2, w3, b3, res, w1, b1 = _seam_operands(B, H, W, P, P2, torch.float16)
    w3, w1 = ops.split_pair(w3.cuda()), ops.split_pair(w1.cuda())
    want_y, want_t1 = ops.conv_c3c1_wpair_keep(t2, w3, b3, res, w1, b1)
    y, t1 = Guarded((B, H, W, 4 * P), torch.float16), Guarded((B, H, W, P2), torch.float16)
    call('dir_conv_c3c1_wpair_keep', ptr(t2), ptr(w3[0]), ptr(w3[1]), ptr(b3), ptr(res), ptr(y.plane), ptr(w1[0]), ptr(w1[1]),
         ptr(b1), ptr(t1.plane), B, H, W, P2, 1, 1, 0, stream_ptr())
    y.check(want_y, 'conv_c3c1_wpair_keep: y')
    t1.check(want_t1, 'conv_c3c1_wpair_keep: t1')


@pytest.mark.experiments      # conv_seam3.hip ships in experiments builds only (DIR_EXPERIMENTS=1 csrc/build.sh)
@pytest.mark.parametrize('dname', list(DTYPES))
def test_layer3_seam_stays_inside_y_and_t1(dname):
    """dir_conv_c3c1 at planes 256 (conv_seam3.hip; whole 64-pixel tiles only: 2 x 8 x 8 = two tiles)."""
    from dirtorch_amd._lib import call, ptr, stream_ptr
    ops = _ops()
    B, H, W, P, P2 = 2, 8, 8, 256, 256
    dt = DTYPES[dname]
    t2, w3, b3, res, w1, b1 = _seam_operands(B, H, W, P, P2, dt)
    w3, w1 = w3.to(dt).cuda(), w1.to(dt).cuda()
    want_y, want_t1 = ops.conv_c3c1(t2, w3, b3, res, w1, b1)
    y, t1 = Guarded((B, H, W, 4 * P), dt), Guarded((B, H, W, P2), dt)
    call('dir_conv_c3c1', ptr(t2), ptr(w3), ptr(b3), ptr(res), ptr(y.plane), ptr(w1), ptr(b1), ptr(t1.plane), B, H, W, P, P2,
         1, 1, ops._dtype_code(t2), stream_ptr())
    y.check(want_y, 'conv_c3c1 planes 256 %s: y' % dname)
    t1.check(want_t1, 'conv_c3c1 planes 256 %s: t1' % dname)

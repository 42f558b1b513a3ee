"""Every (tile variant, split-K factor) pair the conv picker launches, at a real layer shape that lands on it, against an fp32
CPU reference - element by element, in bf16 and fp16 (tests/picker_cases.py holds the table; tests/test_capi_host.py keeps it
in step with the picker).

The operands are exactly representable in both 16-bit formats (bf16-rounded, magnitudes under 2^-14 zeroed), so one fp32
reference of the same values serves both dtypes, and the tolerance is test_ops_gpu.py's check_close: one output rounding
plus summation-order noise.  Each pair is launched the way the engine launches it (the plain entry point when it does not
split), twice - bitwise equal, since neither split-K nor the persistent kernels sum through atomics - and once more with
the library choosing variant and split itself, which must be the same launch.
"""
import functools
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from picker_cases import PICKER_CASES
from test_ops_gpu import DTYPES, RTOL

pytestmark = pytest.mark.gpu

CASES = [(r, d) for r in PICKER_CASES for d in ('bf16', 'fp16')]


def _exact16(t):
    """Round to bf16 and flush what fp16 could not hold as a normal number: the result is exact in both formats."""
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


@functools.lru_cache(maxsize=1)     # (the cases run row by row, bf16 then fp16: one row's operands and reference at a time)
def _operands(row):
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu = row[:11]
    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    OH, OW = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    x = _exact16(torch.randn(B, H, W, Cin, generator=g).clamp_(min=0))                     # post-ReLU activations
    w = _exact16(torch.randn(Cout, k, k, Cin, generator=g) * math.sqrt(2.0 / (k * k * Cin)))   # He-scaled filter
    bias = torch.randn(Cout, generator=g) * 0.2
    res = _exact16(torch.randn(B, OH, OW, Cout, generator=g)) if use_res else None          # signed residual
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), bias, stride, pad)
    if res is not None:
        y = y + res.permute(0, 3, 1, 2)
    if relu:
        y = F.relu(y)
    return x, w, bias, res, y.permute(0, 2, 3, 1).reshape(B * OH * OW, Cout).contiguous()


def _report(got, ref, dname, what, BM, BN):
    """check_close's tolerance; the failure names the bad-element count and the first bad (pixel row m, channel n) with its
    (m // BM, n // BN) tile."""
    err = (got - ref).abs()
    tol = RTOL[dname] * ref.abs() + RTOL[dname] * ref.abs().mean() + 1e-5
    bad = err > tol
    if bad.any():
        idx = bad.nonzero()
        m, n = (int(v) for v in idx[0])
        tiles = {(int(i[0]) // BM, int(i[1]) // BN) for i in idx[:100000]}
        pytest.fail('%s: %d / %d elements out of tolerance (max err %.4g, ref rms %.4g); first bad m = %d, n = %d: got %.5f ref %.5f, '
                    'tile (%d, %d) of %d x %d; %d tiles hold bad elements (of the first 100 000)'
                    % (what, int(bad.sum()), bad.numel(), float(err.max()), float(ref.pow(2).mean().sqrt()), m, n,
                       float(got[m, n]), float(ref[m, n]), m // BM, n // BN, BM, BN, len(tiles)))


@pytest.mark.parametrize('row,dname', CASES, ids=['%s-%s-k%d-%s' % (r[0], r[11], r[12], d) for r, d in CASES])
def test_picked_pair_vs_fp32_reference(row, dname):
    from dirtorch_amd import ops
    tag, B, H, W, Cin, Cout, k, stride, pad, use_res, relu, vname, ks = row
    names = ops.conv_variant_names()
    assert vname in names, vname
    dt = DTYPES[dname]
    x, w, bias, res, ref = _operands(row)
    args = (x.to(dt).cuda(), w.to(dt).cuda(), bias.cuda(), None if res is None else res.to(dt).cuda())
    kw = dict(stride=stride, pad=pad, relu=relu)

    def launch():
        if ks > 1:
            y = ops.conv_bn_act(*args, variant=names.index(vname), ksplit=ks, **kw)
            assert ops.conv_bn_act.last_ksplit == ks
            return y
        return ops.conv_bn_act(*args, variant=names.index(vname), **kw)
    y = launch()
    again = launch()
    auto = ops.conv_bn_act(*args, ksplit=-1, **kw)     # the library's own (variant, ksplit)
    auto_ks = ops.conv_bn_act.last_ksplit
    torch.cuda.synchronize()
    what = '%s %s/%d %s' % (tag, vname, ks, dname)
    BM, BN = (int(v) for v in vname.split('_')[0].split('x'))
    _report(y.float().cpu().reshape(ref.shape), ref, dname, what, BM, BN)
    assert torch.equal(y, again), '%s: two launches differ in %d elements' % (what, int((y != again).sum()))
    assert auto_ks == ks and torch.equal(y, auto), '%s: the library chose ksplit %d and a different result' % (what, auto_ks)

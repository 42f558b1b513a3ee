"""Every launch the tuner can keep, at real layer shapes, bit for bit.

DIRTORCH_AMD_AUTOTUNE=1 / DIRTORCH_AMD_TUNE_CACHE keep, per layer, whichever ADMISSIBLE tile variant timed fastest, in
conv_splitk_factor(variant, shape) K slices - so a tuned run can execute any (layer kind, variant) class the library admits on
the claimed workloads (588 of them; the picker reaches 96), and which one is timing noise.  exact_conv.candidate_table()
computes those classes from the library's own predicates and gives each its smallest and its largest admissible workload shape,
a ragged native / multiscale one, and a shape for every split factor (tests/test_exact_lattice_cpu.py fails, naming the class,
if one has no row).

Per shape and dtype the lattice operands (tests/exact_conv.py: fp32 sums exact in every order) are drawn once on the device;
the naive kernel computes the whole tensor; three whole images of it (first, middle, last) go back to the host and must equal
the CPU reference bit for bit; then every candidate's WHOLE output - launched as the tuner launches it, variant v with the
library's own split factor - and the picker's own pair must equal the naive kernel's on the device.  No element of any output
is left uncompared.
"""
import pytest
import torch

import exact_conv as E

pytestmark = pytest.mark.gpu


def _rows():
    try:
        _, rows, _ = E.candidate_table()
    except Exception:      # (no library at collection time: nothing to parametrise, test_exact_lattice_cpu.py reports it)
        return []
    return [(sh, tag, tuple(vs)) for sh, (tag, vs) in rows.items()]


CASES = [(r, d) for r in _rows() for d in ('bf16', 'fp16')]


@pytest.mark.parametrize('case,dname', CASES, ids=['%s-%dcand-%s' % (r[1], len(r[2]), d) for r, d in CASES])
def test_every_tuner_candidate_equals_the_naive_kernel_bitwise(case, dname):
    from dirtorch_amd import ops
    shape, tag, variants = case
    names = ops.conv_variant_names()
    dt = E.DTYPES[dname]
    row = E.table_row(shape, tag)
    B, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    x, w, bias, res = E.lattice_operands(row, dt, 'cuda')
    kw = dict(stride=stride, pad=pad, relu=relu)
    y0 = ops.conv_bn_act(x, w, bias, res, naive=True, **kw)
    torch.cuda.synchronize()
    what = '%s %r %s' % (tag, shape, dname)
    for b in sorted({0, B // 2, B - 1}):
        want, value = E.exact_reference(x[b:b + 1].cpu(), w.cpu(), bias.cpu(), None if res is None else res[b:b + 1].cpu(),
                                        stride, pad, relu, dt)
        E.report_mismatch(y0[b:b + 1].cpu(), want, what + ': naive kernel vs the CPU, image %d' % b, 64, 64, value)
    failures = []
    launches = [(v, names[v]) for v in variants] + [(-1, 'picker')]
    for v, vname in launches:
        y = ops.conv_bn_act(x, w, bias, res, variant=v, ksplit=-1, **kw)
        ks = ops.conv_bn_act.last_ksplit
        if v >= 0:
            assert ks == E.variant_splitk(v, shape), (vname, ks)
        BM, BN = (int(t) for t in vname.split('_')[0].split('x')) if v >= 0 else (64, 64)
        msg = E.mismatch_report(y, y0, '%s: %s/k%d vs the naive kernel' % (what, vname, ks), BM, BN)
        if msg:
            failures.append(msg)
        del y
    assert not failures, '%d of %d launches differ:\n' % (len(failures), len(launches)) + '\n'.join(failures)

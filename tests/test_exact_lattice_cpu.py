"""The conditions on the INPUTS of the bit-exact conv tests (tests/exact_conv.py), met by the CPU reference alone.

For every row the GPU tests use - the small shapes of test_exact_conv_gpu.py and the tuner-candidate shapes of
test_exact_tuner_candidates_gpu.py:
  * bit_budget holds: every sum a kernel can form fits fp32's 24 significant bits (22 used), stays under fp16's 65 504 and
    above its smallest normal number;
  * the fp32 CPU convolution of the lattice operands equals the fp64 one bit for bit, so it is a valid (and fast) reference;
  * 30-70 % of the outputs are positive (the rest is what the ReLU clamps), at least 30 % of the positive ones cannot be held
    by the target format and at least 2 % are exact ties, in bf16 and in fp16: rounding, tie-breaking and the ReLU are all
    exercised, not just the sum.
A row that misses one is a badly chosen row, to be replaced.  The statistics of a large row are taken on its layer at batch 1 on
a map of at most 40 x 40 (exact_conv.stat_crop): they are a property of K and of the lattice, not of the map.

The candidate table of the tuner tests is gated here too: every (layer kind, variant) class the library admits on the claimed
workloads has a row, and nothing admissible is refused by the launch's size limit.
"""
import functools

import pytest
import torch

import exact_conv as E


def _table():
    try:
        return E.candidate_table()
    except ImportError:
        return {}, {}, []


@functools.lru_cache(maxsize=None)
def _all_plain_rows():
    _, rows, _ = _table()
    return tuple(E.small_plain_rows()) + tuple(E.table_row(sh, tag) for sh, (tag, _) in rows.items())


def _layer_key(row):
    return tuple(E.stat_crop(row)[1:])


@functools.lru_cache(maxsize=None)
def _crop_values(key):
    """fp32 values before the store of the cropped layer; asserts fp32 == fp64."""
    row = ('crop',) + key
    x, w, bias, res = E.lattice_operands(row, torch.float32, seed=E.zlib.crc32(repr(key).encode()))
    stride, pad, relu = key[6], key[7], key[9]
    v32 = E.exact_value(x, w, bias, res, stride, pad, relu)
    v64 = E.exact_value(x, w, bias, res, stride, pad, relu, torch.float64)
    assert torch.equal(v32.double(), v64), 'fp32 and fp64 CPU convolutions differ on lattice operands: %r' % (key,)
    return v32


def _check_stats(value, what):
    for dname, dt in E.DTYPES.items():
        positive, inexact, ties = E.rounding_stats(value, dt)
        assert 0.30 <= positive <= 0.70, '%s %s: %.1f %% of the outputs are positive' % (what, dname, 100 * positive)
        assert inexact >= 0.30, '%s %s: only %.1f %% of the positive outputs need rounding' % (what, dname, 100 * inexact)
        assert ties >= 0.02, '%s %s: only %.2f %% of the positive outputs are exact ties' % (what, dname, 100 * ties)


def test_bit_budget_of_every_row():
    rows = _all_plain_rows()
    assert len(rows) > 40
    worst = 0
    for row in rows:
        worst = max(worst, max(p[3] for p in E.bit_budget(row)))
    for B, H, W, P, P2, ds in E.seam_cases():
        worst = max(worst, max(p[3] for p in E.bit_budget((B, H, W, P, P2, 2 * P if ds else P, not ds), 'seam')))
    assert worst <= E.SUM_BITS <= 24 - 2, worst      # two bits of slack under fp32's 24


def test_bit_budget_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):      # K = 3 x 3 x 2^20: the products alone pass 65 504 and 24 bits
        E.bit_budget(('too_long', 1, 8, 8, 1 << 20, 64, 3, 1, 1, False, True))
    with pytest.raises(AssertionError):      # planes 2048: conv1's sums of the rounded y pass fp16's range
        E.bit_budget((1, 8, 8, 2048, 2048, 2048, True), 'seam')


def test_plain_rows_fp32_is_exact_and_rounding_is_exercised():
    keys = sorted({_layer_key(r) for r in _all_plain_rows()}, key=repr)
    for key in keys:
        _check_stats(_crop_values(key), 'layer %r' % (key,))
    print('%d rows, %d distinct cropped layers checked' % (len(_all_plain_rows()), len(keys)))


@pytest.mark.parametrize('relu3', [True, False])
def test_seam_rows_chain_is_exact_and_rounding_is_exercised(relu3):
    """The seam's final output t1 meets the conditions; its block output y is an integer below 2^10 by construction (what keeps
    conv1's sums exact), so y's own store is compared bit for bit but rarely rounds."""
    for P, P2, ds in sorted({c[3:] for c in E.seam_cases()}):
        t2, w3, b3, other, w1, b1 = E.seam_operands((1, 40, 40, P, P2), torch.float32, seed=P + P2 + ds, ds=ds)
        for dname, dt in E.DTYPES.items():
            args = [t.to(dt) for t in (t2, w3)] + [b3, None if ds else other.to(dt), w1.to(dt), b1, relu3, True, dt]
            y, t1, vy, vt = E.seam_reference(*args, x=other.to(dt) if ds else None)
            assert torch.equal(vy, vy.round()) and float(vy.abs().max()) < 1024
            # fp64 of the same chain from the same rounded y
            v64 = E.exact_value(y, w1.reshape(P2, 1, 1, -1), b1, None, 1, 0, True, torch.float64)
            assert torch.equal(vt.double(), v64)
        _check_stats(vt, 'seam P %d P2 %d ds %d' % (P, P2, ds))


def test_every_tuner_candidate_class_has_a_row():
    """Every (layer kind, variant) class admissible on a shape of picker_cases.workload_layers() is launched somewhere in the
    candidate table, at its smallest and largest admissible workload shape; every distinct split factor of a class has a shape."""
    from dirtorch_amd import ops
    names = ops.conv_variant_names()
    classes, rows, unlaunchable = E.candidate_table()
    assert not unlaunchable, ('admissible by dir_conv_variant_admissible, refused by the launch (size limit): %s'
                              % [(names[c[-1]], c[:5], sh) for c, sh in unlaunchable[:8]])
    covered, splits_covered = {}, set()
    for sh, (tag, vs) in rows.items():
        for v in vs:
            assert E.variant_admissible(v, sh), (names[v], sh)
            covered.setdefault(E.layer_kind(sh) + (v,), []).append(sh)
            splits_covered.add(E.layer_kind(sh) + (v, E.variant_splitk(v, sh)))
    missing = sorted(set(classes) - set(covered))
    assert not missing, 'classes without a row: %s' % [(c[:5], names[c[-1]]) for c in missing]
    order = lambda s: (E._pixels(s), s)
    for cls, shs in classes.items():
        assert min(shs, key=order) in covered[cls] and max(shs, key=order) in covered[cls], (cls[:5], names[cls[-1]])
        for sh in shs:
            ks = E.variant_splitk(cls[-1], sh)
            assert cls + (ks,) in splits_covered, 'split factor %d of %s on %r has no row' % (ks, names[cls[-1]], cls[:5])
    n_cand = sum(len(vs) for _, vs in rows.values())
    print('%d classes (%d layer kinds x %d variants), %d distinct shapes, %d (class, shape) candidates'
          % (len(classes), len({c[:5] for c in classes}), len(names), len(rows), n_cand))
    # the number the library admits today; a new variant or workload changes it, and with it the table - on purpose
    assert len(classes) >= 588


def test_scratch_reserved_for_the_engines_own_split_is_what_the_factor_needs():
    """dir_conv_variant_splitk is the factor dir_conv_heuristic reports for the picker's own variant, 1 where nothing splits."""
    import ctypes
    from dirtorch_amd import _lib, ops
    names = ops.conv_variant_names()
    from picker_cases import PICKER_CASES
    for tag, B, H, W, Cin, Cout, k, stride, pad, res, relu, vname, ks in PICKER_CASES:
        assert E.variant_splitk(names.index(vname), (B, H, W, Cin, Cout, k, stride, pad, res)) == ks, tag
    with pytest.raises(_lib.DirError):       # not admissible: no factor
        E.variant_splitk(names.index('256x64_patchlc3x3'), (1, 8, 8, 128, 128, 1, 1, 0, False))
    with pytest.raises(_lib.DirError):
        _lib.call('dir_conv_variant_splitk', 0, 1, 8, 8, 64, 64, 1, 1, 1, 0, 8, 8, 0, ctypes.POINTER(ctypes.c_int)())

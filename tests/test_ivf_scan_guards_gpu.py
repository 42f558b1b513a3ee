"""The guards the three list-major scans share (csrc/ivf_scan.h), met directly for every format: the workgroups of a grid
that is only an upper bound return at once, and a stated width below the reach of the slots stores nothing at or past it.

D = 64: one slab for the int8 and the sign-bit scan (half of it query codes), a quarter slab for fp4; the query rows lie
at their smallest pitch, so an uncut query chunk would be the next query's codes.  Four lists of 0, 1, 257 and 40 rows:
list 2 has two tiles, the second of one row.  33 queries with two slots each: slot 0 of every query is list 2 - two
groups, the second of one pair; slot 1 is list 3 for five queries, the empty list 0 for one, -1 for one, and list 1 for
the rest, so every slot of the table says something.  The slots of a query lie GAP columns apart.  The outputs are PAST
columns wider than the stated width and pre-filled with FILL; expected scores are index_ref / fp4_ref / bin_ref on the
CPU, compared on bits."""
import numpy as np
import pytest
import torch

import bin_ref
import fp4_ref
import index_ref
from index_util import cuda as _cuda
from topk_ref import bits

pytestmark = pytest.mark.gpu

D = 64
LENS = [0, 1, 257, 40]
NROWS = sum(LENS)
LIST_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
Q, GAP, PAST, FILL = 33, 2, 9, 12345
SURPLUS, SHORT = 5, 7                   # workgroups added to the grid; columns the stated width lacks to the reach


def _table():
    probe = np.full((Q, 2), 1, np.int32)
    probe[:, 0] = 2
    probe[[3, 8, 17, 31, 32], 1] = 3    # (32 is the one pair of list 2's second group)
    probe[5, 1] = 0
    probe[11, 1] = -1
    plen = np.where(probe >= 0, np.array(LENS)[np.maximum(probe, 0)], 0)
    col_off = (np.cumsum(plen + GAP, axis=1) - plen - GAP).astype(np.int32)
    return probe, col_off, int((col_off + plen).max())


def _fp4_rows(r, n):
    ldc, lde = fp4_ref.widths(D)
    nib = r.randint(0, 16, (n, 2 * ldc)).astype(np.uint8)
    exps = np.full((n, lde), 127, np.uint8)
    exps[:, :D // 32] = r.randint(125, 128, (n, D // 32))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), exps


def _case(fmt):
    """(the flat scores [Q, NROWS] of the restatement, scan(**kw) -> ops.ivf_scan*'s result on the device copies)"""
    from dirtorch_amd import ops
    r = np.random.RandomState({'i8': 411, 'fp4': 412, 'bin': 413}[fmt])
    sq = np.exp(r.uniform(-4, 2, Q)).astype(np.float32)
    sb = np.exp(r.uniform(-4, 2, NROWS)).astype(np.float32)
    ids = r.permutation(NROWS).astype(np.int32)
    tail = (_cuda(ids, np.int32), _cuda(LIST_OFF, np.int32))
    if fmt == 'fp4':
        (cq, eq), (cb, eb) = _fp4_rows(r, Q), _fp4_rows(r, NROWS)
        want = fp4_ref.score(cq, eq, sq, cb, eb, sb, D)
        dev = (_cuda(cq, np.uint8), _cuda(eq, np.uint8), _cuda(sq), _cuda(cb, np.uint8), _cuda(eb, np.uint8), _cuda(sb)) + tail
        return want, ids, lambda probe, col_off, **kw: ops.ivf_scan_fp4(*dev, probe, col_off, D, **kw)
    qc = r.randint(-127, 128, (Q, D)).astype(np.int8)
    if fmt == 'i8':
        cb = r.randint(-127, 128, (NROWS, D)).astype(np.int8)
        want = index_ref.score(qc, sq, cb, sb)
        dev = (_cuda(qc, np.int8), _cuda(sq), _cuda(cb, np.int8), _cuda(sb)) + tail
        return want, ids, lambda probe, col_off, **kw: ops.ivf_scan(*dev, probe, col_off, D, **kw)
    rows = r.randint(0, 256, (NROWS, bin_ref.width(D))).astype(np.uint8)
    want = bin_ref.score(qc, sq, rows, sb, D)
    dev = (_cuda(qc, np.int8), _cuda(sq), _cuda(rows, np.uint8), _cuda(sb)) + tail
    return want, ids, lambda probe, col_off, **kw: ops.ivf_scan_bin(*dev, probe, col_off, D, **kw)


def _expected(want, ids, probe, col_off, width):
    """ids [Q, width] (-1 where no slot covers), scores and which of them a slot covers - what lies below `width` only"""
    exp_ids = np.full((Q, width), -1, np.int32)
    exp_scores = np.zeros((Q, width), np.float32)
    covered = np.zeros((Q, width), bool)
    for q in range(Q):
        for p in range(probe.shape[1]):
            l = probe[q, p]
            if l >= 0:
                n = max(0, min(LENS[l], width - col_off[q, p]))
                cols, rows = slice(col_off[q, p], col_off[q, p] + n), slice(LIST_OFF[l], LIST_OFF[l] + n)
                exp_ids[q, cols], exp_scores[q, cols], covered[q, cols] = ids[rows], want[q, rows], True
    return exp_ids, exp_scores, covered


def _check(scan, want, ids, probe, col_off, width, **kw):
    scores = torch.full((Q, width + PAST), float(FILL), dtype=torch.float32, device='cuda')
    out_ids = torch.full((Q, width + PAST), FILL, dtype=torch.int32, device='cuda')
    got_s, got_i = scan(_cuda(probe, np.int32), _cuda(col_off, np.int32), width=width, out=(scores, out_ids), **kw)
    assert got_s.data_ptr() == scores.data_ptr() and tuple(got_s.shape) == (Q, width) == tuple(got_i.shape)
    gi, gs = out_ids.cpu().numpy(), scores.cpu().numpy()
    exp_ids, exp_scores, covered = _expected(want, ids, probe, col_off, width)
    assert (gi[:, :width] == exp_ids).all(), np.argwhere(gi[:, :width] != exp_ids)[:5]
    ok = bits(gs[:, :width]) == bits(exp_scores)
    assert ok[covered].all(), np.argwhere(~ok & covered)[:5]
    assert (gi[:, width:] == FILL).all() and (gs[:, width:] == FILL).all()        # nothing at or past the width, in either array
    return gi[:, :width], gs[:, :width], covered


@pytest.mark.parametrize('fmt', ['i8', 'fp4', 'bin'])
def test_surplus_workgroups_and_a_short_width(fmt):
    from dirtorch_amd import ops
    want, ids, scan = _case(fmt)
    probe, col_off, reach = _table()
    assert reach == LENS[2] + GAP + LENS[3]
    tables = ops.ivf_probe_tables(_cuda(LIST_OFF, np.int32), _cuda(probe, np.int32), _cuda(col_off, np.int32))
    # list 1: one tile, one group; list 2: two tiles of two groups; list 3: one tile, one group; the empty list 0: none
    assert tables[4] == 1 + 2 * 2 + 1 and tables[5] == reach
    plain = _check(scan, want, ids, probe, col_off, reach, tables=tables)
    # (a) a grid SURPLUS workgroups above item_off[nlist]: they return at once, the results are the same
    raised = _check(scan, want, ids, probe, col_off, reach, tables=tables[:4] + (tables[4] + SURPLUS, tables[5]))
    assert (raised[0] == plain[0]).all() and (bits(raised[1]) == bits(plain[1]))[plain[2]].all()
    # (b) a stated width SHORT columns below the reach: the rows of list 3 past it are not stored
    short = _check(scan, want, ids, probe, col_off, reach - SHORT)
    assert (short[0] == plain[0][:, :reach - SHORT]).all() and short[2][3, -1] and not short[2][0, -1]

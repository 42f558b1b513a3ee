"""Class-labelled ranking on the device (dir_label_rank, ranking.eval_labelled_device, eval_dir.eval_model)
against the numpy fp64 restatement of tests/label_rank_ref.py on the same score tensor.

Tolerance: 1e-12 absolute on AP - at most ~10^4 fp64 terms in [0, 1/n_pos], each rounded once, so two summation orders
differ by < 1e-15, while ONE miscounted item moves an AP by at least 1/(n_pos * N) > 1e-9 at every shape below.
best_rank is compared exactly."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from label_rank_ref import csr_tables, label_rank_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AP_TOL = 1e-12


def _cuda(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _run(scores, labels, C, qclass, qself, lds=None):
    """(ap, best_rank) ndarrays of ops.label_rank on host arrays; lds > N puts the rows into a wider buffer."""
    from dirtorch_amd import ops
    scores = np.asarray(scores, np.float32)
    Q, N = scores.shape
    off, members = csr_tables(labels, C)
    if lds is None:
        dev = _cuda(scores, np.float32)
    else:
        wide = torch.full((Q, lds), float('nan'), dtype=torch.float32, device='cuda')   # the padding must not be read
        wide[:, :N] = _cuda(scores, np.float32)
        dev = wide[:, :N]
    ap, best = ops.label_rank(dev, _cuda(labels), _cuda(off), _cuda(members), _cuda(qclass), _cuda(qself))
    assert ap.dtype == torch.float64 and best.dtype == torch.int32 and ap.is_cuda and best.is_cuda
    return ap.cpu().numpy(), best.cpu().numpy()


def _check(scores, labels, C, qclass, qself, lds=None):
    ap, best = _run(scores, labels, C, qclass, qself, lds)
    want_ap, want_best = label_rank_ref(scores, labels, qclass, qself)
    print('max |AP - ref| = %.3g' % np.nanmax(np.abs(ap - want_ap)) if len(ap) else 'empty')
    assert (np.isnan(ap) == np.isnan(want_ap)).all(), (ap, want_ap)
    ok = ~np.isnan(want_ap)
    assert (np.abs(ap[ok] - want_ap[ok]) <= AP_TOL).all(), np.abs(ap[ok] - want_ap[ok]).max()
    assert (best == want_best).all(), (best, want_best)
    return ap, best


def test_score_chunk_boundary_ragged_tail_and_row_stride():
    r = np.random.RandomState(21)
    N, Q, C = 16384 + 37, 5, 40
    labels = r.randint(0, C, N)
    scores = r.standard_normal((Q, N)).astype(np.float32)
    scores[1] = np.round(scores[1] * 8) / 8                     # a row with ties
    qself = np.array([3, -1, N - 1, -1, 16384], np.int32)       # last item, and the first item past the boundary
    qclass = labels[[3, 100, N - 1, 7, 16384]].astype(np.int32)
    _check(scores, labels, C, qclass, qself, lds=N + 11)


def test_class_larger_than_one_slice():
    r = np.random.RandomState(22)
    N, C = 9000, 30
    labels = r.randint(1, C, N)
    big = r.choice(N, 4100, replace=False)                      # class 0: 4100 members, past the 4096 slice
    labels[big] = 0
    scores = (r.standard_normal((3, N)) + (labels == 0) * 0.5).astype(np.float32)
    scores[1] = np.round(scores[1] * 16) / 16
    qclass = np.array([0, 0, 5], np.int32)
    qself = np.array([int(big[7]), -1, -1], np.int32)
    ap, _ = _check(scores, labels, C, qclass, qself)
    assert (ap > 0).all()


def test_three_score_levels_and_signed_zero():
    r = np.random.RandomState(23)
    N, Q, C = 3000, 4, 9
    labels = r.randint(0, C, N)
    scores = r.randint(-1, 2, (Q, N)).astype(np.float32)        # {-1, 0, 1}: everything ties
    qclass = labels[[0, 1, 2, 3]].astype(np.int32)
    qself = np.array([0, -1, 2, -1], np.int32)
    plus = _check(scores, labels, C, qclass, qself)
    minus_scores = scores.copy()
    zeros = np.flatnonzero(scores.ravel() == 0)
    minus_scores.ravel()[zeros[::3]] = -0.0
    assert np.signbit(minus_scores).sum() > (scores < 0).sum()
    minus = _check(minus_scores, labels, C, qclass, qself)
    assert (plus[0] == minus[0]).all() and (plus[1] == minus[1]).all()


def test_lonely_class_and_absent_class():
    r = np.random.RandomState(24)
    N, C = 500, 6
    labels = r.randint(0, C - 1, N)
    labels[123] = C - 1                                         # class 5: one image
    scores = r.standard_normal((3, N)).astype(np.float32)
    scores[:2, 123] = scores[:2].max(axis=1) + 1                # ... which scores best
    qclass = np.array([C - 1, C - 1, -1], np.int32)
    qself = np.array([123, -1, -1], np.int32)
    ap, best = _check(scores, labels, C, qclass, qself)
    assert ap.tolist() == [-1.0, 1.0, -1.0] and best.tolist() == [0, 0, N]


def test_non_finite_scores():
    r = np.random.RandomState(25)
    N, C = 700, 5
    labels = r.randint(0, C, N)
    scores = r.standard_normal((7, N)).astype(np.float32)
    qclass = np.full(7, 2, np.int32)
    qself = np.array([-1, -1, -1, 40, 41, -1, -1], np.int32)
    labels[40] = labels[41] = 2
    members = np.setdiff1d(np.flatnonzero(labels == 2), [40, 41])
    others = np.flatnonzero(labels != 2)
    scores[0, others[5]] = np.nan                               # a NaN negative
    scores[1, members[3]] = np.inf                              # +inf on a positive: it places first
    scores[2, labels == 2] = np.nan                             # every image of the class NaN: the first of them, after all numbers
    scores[3, 40] = np.nan                                      # the only non-finite score is the query's own: finite AP
    scores[4, 41] = -np.inf
    scores[5, members[0]] = np.nan                              # a NaN positive
    ap, best = _check(scores, labels, C, qclass, qself)
    assert np.isnan(ap).tolist() == [True, True, True, False, False, True, False]
    assert best[1] == 0 and best[2] == N - len(np.flatnonzero(labels == 2))


def test_one_image_and_no_query():
    from dirtorch_amd import ops
    ap, best = _check(np.array([[0.25]], np.float32), np.array([0]), 1, np.array([0], np.int32), np.array([-1], np.int32))
    assert ap.tolist() == [1.0] and best.tolist() == [0]
    ap, best = _check(np.array([[0.25]], np.float32), np.array([0]), 1, np.array([0], np.int32), np.array([0], np.int32))
    assert ap.tolist() == [-1.0] and best.tolist() == [0]
    empty = torch.empty(0, 5, dtype=torch.float32, device='cuda')
    off, members = csr_tables(np.zeros(5, np.int64), 1)
    none = torch.empty(0, dtype=torch.int32, device='cuda')
    ap, best = ops.label_rank(empty, _cuda(np.zeros(5)), _cuda(off), _cuda(members), none, none)
    assert ap.shape == (0,) and best.shape == (0,) and ap.dtype == torch.float64 and best.dtype == torch.int32


def test_two_runs_are_bit_identical():
    from dirtorch_amd import ops
    r = np.random.RandomState(26)
    N, Q, C = 5000, 64, 12
    labels = r.randint(0, C, N)
    off, members = csr_tables(labels, C)
    scores = _cuda(np.round(r.standard_normal((Q, N)) * 32) / 32, np.float32)
    args = (_cuda(labels), _cuda(off), _cuda(members), _cuda(labels[:Q]), _cuda(np.arange(Q)))
    a1, b1 = ops.label_rank(scores, *args)
    a2, b2 = ops.label_rank(scores, *args)
    assert torch.equal(a1, a2) and torch.equal(b1, b2)
    assert float(a1.min()) > 0


def test_invalid_arguments_raise():
    from dirtorch_amd import _lib, ops
    from dirtorch_amd._lib import ptr, stream_ptr
    r = np.random.RandomState(27)
    N, Q, C = 300, 4, 5
    labels = r.randint(0, C, N)
    off, members = csr_tables(labels, C)
    scores = _cuda(r.standard_normal((Q, N)), np.float32)
    qclass, qself = labels[:Q].astype(np.int32), -np.ones(Q, np.int32)
    good = dict(labels=labels, off=off, members=members, qclass=qclass, qself=qself)

    def run(**change):
        a = dict(good, **change)
        return ops.label_rank(scores, _cuda(a['labels']), _cuda(a['off']), _cuda(a['members']), _cuda(a['qclass']),
                              _cuda(a['qself']))
    run()
    for bad_member in (N, -1):
        m = members.copy()
        m[17] = bad_member
        with pytest.raises(_lib.DirError, match='class_members'):
            run(members=m)
    swapped = members.copy()
    swapped[[0, N - 1]] = swapped[[N - 1, 0]]                    # filed under another class than labels gives them
    with pytest.raises(_lib.DirError, match='class_members'):
        run(members=swapped)
    with pytest.raises(_lib.DirError, match='qclass'):
        run(qclass=np.array([0, C, 1, 2], np.int32))
    with pytest.raises(_lib.DirError, match='qself'):
        run(qself=np.array([-1, N, -1, -1], np.int32))
    broken = off.copy()
    broken[2] = broken[3] + 1
    with pytest.raises(_lib.DirError, match='class_off'):
        run(off=broken)
    short = off.copy()
    short[C] -= 1                                               # the last image of the last class is not listed
    with pytest.raises(_lib.DirError, match='class_off'):
        run(off=short)
    twice = members.copy()
    twice[1] = twice[0]                                         # same class, one image listed twice, its neighbour never
    assert labels[members[0]] == labels[members[1]]
    with pytest.raises(_lib.DirError, match='twice'):
        run(members=twice)
    ap = torch.empty(Q, dtype=torch.float64, device='cuda')
    best = torch.empty(Q, dtype=torch.int32, device='cuda')
    t = [_cuda(x) for x in (labels, off, members, qclass, qself)]
    with pytest.raises(_lib.DirError, match='lds'):
        _lib.call('dir_label_rank', ptr(scores), N - 1, Q, N, ptr(t[0]), ptr(t[1]), ptr(t[2]), C, ptr(t[3]), ptr(t[4]),
                  ptr(ap), ptr(best), stream_ptr())
    with pytest.raises(_lib.DirError, match='null'):
        _lib.call('dir_label_rank', ctypes.c_void_p(0), N, Q, N, ptr(t[0]), ptr(t[1]), ptr(t[2]), C, ptr(t[3]), ptr(t[4]),
                  ptr(ap), ptr(best), stream_ptr())
    run()                                                       # the library is still usable


# ---- ranking.eval_labelled_device ------------------------------------------------------------------------------------
def _labelled_db(tmp_path, labels, qlabels=None):
    from dirtorch_amd import datasets
    lst = os.path.join(str(tmp_path), 'db.txt')
    with open(lst, 'w') as f:
        f.write(''.join('img%d.jpg c%d\n' % (i, l) for i, l in enumerate(labels)))
    if qlabels is None:
        return datasets.ImageListLabels(lst, root=str(tmp_path))
    qlst = os.path.join(str(tmp_path), 'q.txt')
    with open(qlst, 'w') as f:
        f.write(''.join('q%d.jpg c%d\n' % (i, l) for i, l in enumerate(qlabels)))
    return datasets.ImageListLabelsQ(lst, qlst, root=str(tmp_path))


def _tie_free_descriptors(N, D, first_seed):
    """L2-normalised descriptors whose self-similarity rows have no tie among their 101 best scores: the host's
    np.argsort(-scores) is not stable, so a tie at a top-k boundary would leave ITS answer undefined.  Redrawn with the
    next seed until no row ties (no row is ever left out of the comparison)."""
    from dirtorch_amd import ranking
    for seed in range(first_seed, first_seed + 20):
        x = np.random.RandomState(seed).standard_normal((N, D)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        scores = ranking.similarity_device(x, x).cpu().numpy()
        top = -np.sort(-scores, axis=1)[:, :102]
        if (np.diff(top, axis=1) < 0).all():
            return x, scores
    raise AssertionError('no tie-free draw in 20 seeds')


def test_eval_labelled_device_chunked_equals_one_chunk_and_the_host_loop(tmp_path):
    from dirtorch_amd import ranking
    r = np.random.RandomState(31)
    N, D = 600, 64
    labels = r.randint(0, 25, N)
    labels[77] = 25                                             # a query without positives: AP -1
    db = _labelled_db(tmp_path, labels)
    x, scores = _tie_free_descriptors(N, D, 32)
    aps1, tops1 = ranking.eval_labelled_device(db, x, x)
    aps3, tops3 = ranking.eval_labelled_device(db, x, x, scratch_bytes=4 * N * 200)      # 200 rows per chunk: 3 chunks
    aps7, tops7 = ranking.eval_labelled_device(db, x, x, tables=ranking.build_label_tables(db), scratch_bytes=4 * N * 89)
    assert aps1 == aps3 == aps7 and tops1 == tops3 == tops7
    assert len(aps1) == N and aps1[77] == -1 and all(type(a) is float for a in aps1 if a != -1)
    want_aps = [db.eval_query_AP(q, s) for q, s in enumerate(scores)]
    want_tops = [db.eval_query_top(q, s) for q, s in enumerate(scores)]
    print('max |AP - host| = %.3g' % max(abs(a - b) for a, b in zip(aps1, want_aps)))
    assert all((a == -1) == (b == -1) and abs(a - b) <= AP_TOL for a, b in zip(aps1, want_aps))
    assert tops1 == want_tops and list(tops1[0]) == [1, 5, 10, 20, 50, 100]
    # a query set of its own, one of its classes absent from the database; k above N is dropped like on the host
    dbq = _labelled_db(tmp_path, labels[:90], qlabels=[3, 99, 25, 7])
    qa, qt = ranking.eval_labelled_device(dbq, x[100:104], x[:90], k=(1, 5, 89, 90, 100))
    qs = ranking.similarity_device(x[100:104], x[:90]).cpu().numpy()
    assert qa[1] == -1 and qt[1] == {1: 0.0, 5: 0.0, 89: 0.0}
    assert all(abs(a - dbq.eval_query_AP(q, qs[q])) <= AP_TOL for q, a in enumerate(qa))
    assert qt == [dbq.eval_query_top(q, qs[q], k=(1, 5, 89, 90, 100)) for q in range(4)]
    bad = x.copy()
    bad[5, 0] = np.nan
    with pytest.raises(ValueError, match='query 0'):
        ranking.eval_labelled_device(db, x, bad)


_CHILD = r'''
import json, sys
sys.path[:0] = [%(pkg)r]
from dirtorch_amd import datasets, eval_dir, ranking
calls, device_route = [], ranking.eval_labelled_device
ranking.eval_labelled_device = lambda *a, **kw: (calls.append(1), device_route(*a, **kw))[1]
db = datasets.ImageListLabels(%(lst)r, root=%(root)r)
res = eval_dir.eval_model(db, None, '', detailed=True, load_feats=%(root)r)
json.dump({'res': res, 'device_calls': len(calls)}, open(%(out)r, 'w'))
'''


def test_eval_model_takes_the_device_route_under_the_switch(tmp_path):
    """One fresh process per value of DIRTORCH_AMD_DEVICE_RANK, as in a real run: =1 sends a labelled dataset through
    eval_labelled_device, =0 through the host loop, on the same saved descriptors (load_feats)."""
    r = np.random.RandomState(41)
    N, D = 300, 32
    labels = r.randint(0, 12, N)
    labels[11] = 12
    db = _labelled_db(tmp_path, labels)
    x, _ = _tie_free_descriptors(N, D, 42)
    np.save(os.path.join(str(tmp_path), 'feats.bdescs.npy'), x)
    res = {}
    for flag in ('1', '0'):
        out = os.path.join(str(tmp_path), 'res%s.json' % flag)
        code = _CHILD % dict(pkg=os.path.join(ROOT, 'deep-image-retrieval_amd'), lst=os.path.join(str(tmp_path), 'db.txt'),
                             root=str(tmp_path), out=out)
        subprocess.run([sys.executable, '-c', code], check=True, env=dict(os.environ, DIRTORCH_AMD_DEVICE_RANK=flag),
                       timeout=300)
        res[flag] = json.load(open(out))
    assert res['1']['device_calls'] == 1 and res['0']['device_calls'] == 0
    dev, host = res['1']['res'], res['0']['res']
    assert list(dev) == list(host) and 'mAP' in dev and 'top1' in dev and 'tops' in dev and 'APs' in dev
    print('|mAP device - host| = %.3g' % abs(dev['mAP'] - host['mAP']))
    assert abs(dev['mAP'] - host['mAP']) <= AP_TOL
    assert max(abs(a - b) for a, b in zip(dev['APs'], host['APs'])) <= AP_TOL and dev['APs'][11] == -1
    for key in host:
        if key.startswith('top'):
            assert dev[key] == host[key], key
    assert len(db) == N

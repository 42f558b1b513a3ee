"""Class-labelled ranking, host side (no GPU): the numpy restatement the GPU tests compare against (tests/label_rank_ref.py)
is pinned to sklearn and to the stable argsort it restates, and ranking.build_label_tables to the datasets' own ground
truth (Dataset.get_query_groundtruth)."""
import os

import numpy as np
import pytest

from label_rank_ref import ap_ref, best_rank_ref


def _tie_heavy_rows():
    """(scores fp32 [N], positive [N]) over score levels x positive rates, some zeros written as -0.0."""
    r = np.random.RandomState(11)
    for levels in (2, 3, 7, 50, 10 ** 5):
        for rate in (0.002, 0.01, 0.1, 0.5):
            for N in (1500, 2003):
                s = (r.randint(0, levels, N) - levels // 2).astype(np.float32) / np.float32(levels)
                zeros = np.flatnonzero(s == 0)
                s[zeros[::2]] = -0.0
                pos = r.rand(N) < rate
                pos[r.randint(N)] = True
                yield s, pos


def test_restatement_agrees_with_sklearn_on_tie_heavy_rows():
    sk = pytest.importorskip('sklearn.metrics')
    n = 0
    for s, pos in _tie_heavy_rows():
        want = sk.average_precision_score(pos, s)
        assert abs(ap_ref(s, pos) - want) <= 1e-12, (n, ap_ref(s, pos), want)
        keep = np.ones(len(s), bool)
        keep[np.flatnonzero(pos)[0]] = False          # the query itself: a positive that is left out
        if pos[keep].any():
            assert abs(ap_ref(s, pos, keep) - sk.average_precision_score(pos[keep], s[keep])) <= 1e-12
        n += 1
    assert n == 40
    assert ap_ref(np.zeros(5, np.float32), np.zeros(5, bool)) == -1.0
    bad = np.array([0.5, np.nan, 0.25], np.float32)
    assert np.isnan(ap_ref(bad, [True, False, False]))
    with pytest.raises(ValueError):
        sk.average_precision_score([True, False, False], bad)
    assert ap_ref(bad, [True, False, False], keep=np.array([True, False, True])) == 1.0


def test_restatement_agrees_with_the_stable_argsort():
    r = np.random.RandomState(12)
    for levels in (2, 3, 7, 10 ** 5):
        for N in (1, 2, 257, 1200):
            for nan_rate in (0.0, 0.05, 1.0):
                s = (r.randint(0, levels, N) - levels // 2).astype(np.float32)
                s[r.rand(N) < 0.1] = -0.0
                s[r.rand(N) < nan_rate] = np.nan
                for rate in (0.0, 0.01, 0.3):
                    correct = r.rand(N) < rate
                    rank = best_rank_ref(s, correct)
                    order = np.argsort(-s, kind='stable')
                    assert rank == (N if not correct.any() else int(np.flatnonzero(correct[order])[0]))
                    for k in (k for k in (1, 5, 10, 100) if k <= N):     # (eval_query_top only asks for k < N)
                        assert (rank < k) == bool(correct[order][:k].any())


def _write_pairs(path, keys, labels):
    with open(path, 'w') as f:
        f.write(''.join('%s %s\n' % kv for kv in zip(keys, labels)))


def _check_tables(db, t):
    query_db = db.get_query_db()
    same = query_db is db
    N, Q = len(db), len(query_db)
    assert t['same_set'] == same and t['C'] == len(db.c_relevant_idx)
    for name in ('labels', 'class_off', 'class_members', 'qclass', 'qself'):
        assert t[name].dtype == np.int32, name
    assert t['labels'].shape == (N,) and t['class_members'].shape == (N,) and t['class_off'].shape == (t['C'] + 1,)
    assert t['qclass'].shape == (Q,) and t['qself'].shape == (Q,)
    assert t['class_off'][0] == 0 and t['class_off'][-1] == N and (np.diff(t['class_off']) >= 0).all()
    for c in range(t['C']):
        members = t['class_members'][t['class_off'][c]:t['class_off'][c + 1]]
        assert (t['labels'][members] == c).all() and len(set(members.tolist())) == len(members)
    assert (t['qself'] == (np.arange(Q) if same else -1)).all()
    for q in range(Q):
        gt = db.get_query_groundtruth(q, 'AP')
        c = t['qclass'][q]
        positives = np.zeros(N, bool)
        if c >= 0:
            positives[t['class_members'][t['class_off'][c]:t['class_off'][c + 1]]] = True
        if t['qself'][q] >= 0:
            positives[t['qself'][q]] = False
        assert (positives == (gt > 0)).all(), q
        assert ((gt == 0) == (np.arange(N) == t['qself'][q])).all(), q
        # the top-k side: the images eval_query_top calls correct
        correct = np.array([l == db.get_query_groundtruth(q, 'label') for l in db.labels], dtype=bool)
        assert (correct == (t['labels'] == c)).all(), q


def test_build_label_tables_matches_the_ground_truth(tmp_path):
    from dirtorch_amd import datasets, ranking
    r = np.random.RandomState(13)
    names = ['tower', 'bridge', 'gate', 'lone']
    labels = [names[i] for i in r.randint(0, 3, 40)] + ['lone']      # 'lone': a class whose only image is its own query
    lst = os.path.join(str(tmp_path), 'db.txt')
    _write_pairs(lst, ['img%d.jpg' % i for i in range(len(labels))], labels)
    db = datasets.ImageListLabels(lst, root=str(tmp_path))
    t = ranking.build_label_tables(db)
    _check_tables(db, t)
    assert t['C'] == 4 and (t['qclass'] >= 0).all()

    qlabels = ['gate', 'absent', 'tower', 'absent', 'lone']          # 'absent': no database image carries it
    qlst = os.path.join(str(tmp_path), 'q.txt')
    _write_pairs(qlst, ['q%d.jpg' % i for i in range(len(qlabels))], qlabels)
    dbq = datasets.ImageListLabelsQ(lst, qlst, root=str(tmp_path))
    tq = ranking.build_label_tables(dbq)
    _check_tables(dbq, tq)
    assert tq['qclass'].tolist()[1] == -1 and tq['qclass'].tolist()[3] == -1 and (tq['qself'] == -1).all()
    assert dbq.eval_query_AP(1, np.zeros(len(dbq), np.float32)) == -1

"""The inverted-file int8 index, host side (no GPU): the library exports the new entry points and checks their arguments
before anything is launched, the numpy restatement (tests/ivf_ref.py) agrees with a plain loop over index_ref.score and
topk_ref, and the fixtures of tests/test_ivf_gpu.py have the properties those tests rely on."""
import ctypes

import numpy as np
import pytest

import index_ref
import ivf_ref
from synth import synth_descriptors
from topk_ref import bits, topk_ref_rows


def test_library_exports_the_ivf_entry_points():
    from dirtorch_amd import _lib
    lib = _lib.load()
    for name in ('dir_segment_sums', 'dir_ivf_scan_i8'):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES, 'no ctypes signature for ' + name
    assert len(_lib.SIGNATURES['dir_segment_sums'][1]) == 10 and len(_lib.SIGNATURES['dir_ivf_scan_i8'][1]) == 22


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lib.dir_last_error

    def sums(X=p, ldx=200, N=5, D=200, order=p, seg_off=p, S=3, out=p, lds=200):
        return lib.dir_segment_sums(X, ldx, N, D, order, seg_off, S, out, lds, None)

    assert sums(D=0) == -1 and b'D < 1' in err()
    assert sums(ldx=199) == -1 and sums(lds=199) == -1 and b'ld' in err()
    assert sums(N=-1) == -1 and sums(S=-1) == -1 and b'negative' in err()
    for name in ('X', 'order', 'seg_off', 'out'):
        assert sums(**{name: None}) == -1 and b'null' in err(), name
    assert sums(S=70000) == -1 and b'65535' in err()
    assert sums(S=0) == 0

    def scan(qc=p, ldq=256, qs=p, Q=3, bc=p, ldb=256, bs=p, ids=p, N=40, D=200, list_off=p, nlist=4, pair_off=p, pair_q=p,
             pair_col=p, item_off=p, items=2, scores=p, out_ids=p, lds=64, width=50):
        return lib.dir_ivf_scan_i8(qc, ldq, qs, Q, bc, ldb, bs, ids, N, D, list_off, nlist, pair_off, pair_q, pair_col, item_off,
                                   items, scores, out_ids, lds, width, None)

    assert scan(D=0) == -1 and b'D < 1' in err()
    assert scan(D=131073, ldq=131136, ldb=131136) == -1 and b'exceeds' in err()
    assert scan(ldq=200) == -1 and scan(ldb=200) == -1 and b'ld' in err()       # below D rounded up to 64
    assert scan(lds=49) == -1 and b'lds' in err()
    for name in ('Q', 'N', 'nlist', 'items', 'width'):
        assert scan(**{name: -1}) == -1 and b'negative' in err(), name
    for name in ('qc', 'qs', 'bc', 'bs', 'ids', 'list_off', 'pair_off', 'pair_q', 'pair_col', 'item_off', 'scores', 'out_ids'):
        assert scan(**{name: None}) == -1 and b'null' in err(), name
    assert scan(ldb=264) == -1 and scan(ldq=264) == -1 and b'16' in err()        # the scan moves 16-byte pieces
    assert scan(nlist=0) == -1
    assert scan(Q=0) == 0 and scan(width=0, lds=0) == 0                          # nothing to do: DIR_OK, nothing launched


# ---- the restatement against a plain loop ------------------------------------------------------------------------------
def test_restatement_agrees_with_a_plain_loop():
    """Assignment, probing and the masked search of ivf_ref, one row and one query at a time over index_ref.score and
    topk_ref_rows; a zero row and a non-finite row land in the last list."""
    r = np.random.RandomState(150)
    D, nlist, k = 40, 5, 12
    x = synth_descriptors(8, 90, D)
    x[3] = 0
    x[7, 5] = np.nan
    q = synth_descriptors(9, 11, D)
    centroids = synth_descriptors(10, nlist, D)
    cc, cs = index_ref.quantize(centroids)
    bc, bs = index_ref.quantize(x)
    qc, qs = index_ref.quantize(q)
    lists = np.array([topk_ref_rows(index_ref.score(bc[i:i + 1, :D], bs[i:i + 1], cc[:, :D], cs), 1)[0][0, 0] for i in range(len(x))])
    assert (ivf_ref.assign(bc, bs, centroids) == lists).all()
    assert lists[3] == nlist - 1 and lists[7] == nlist - 1
    store = ivf_ref.build(x, centroids)
    assert store['list_off'][0] == 0 and store['list_off'][-1] == len(x) and sorted(store['ids'].tolist()) == list(range(len(x)))
    for l in range(nlist):
        members = store['ids'][store['list_off'][l]:store['list_off'][l + 1]]
        assert (np.diff(members) > 0).all() and (lists[members] == l).all()
    assert (store['codes'] == bc[store['ids']]).all() and (bits(store['scales']) == bits(bs[store['ids']])).all()
    own = r.randint(0, len(x), len(q)).astype(np.int32)
    for nprobe in (1, 2, nlist):
        probed = ivf_ref.probe(qc, qs, centroids, nprobe)
        for exclude in (None, own):
            got = ivf_ref.search(q, x, centroids, k, nprobe, exclude=exclude)
            for i in range(len(q)):
                pl = topk_ref_rows(index_ref.score(qc[i:i + 1, :D], qs[i:i + 1], cc[:, :D], cs), nprobe)[0][0]
                assert (probed[i] == pl).all()
                cand = np.concatenate([store['ids'][store['list_off'][l]:store['list_off'][l + 1]] for l in pl])
                s = index_ref.score(qc[i:i + 1, :D], qs[i:i + 1], bc[cand][:, :D], bs[cand])
                want = topk_ref_rows(s, k, ids=cand[None].astype(np.int32), exclude=None if exclude is None else exclude[i:i + 1])
                assert (got[0][i] == want[0][0]).all() and (bits(got[1][i]) == bits(want[1][0])).all(), (nprobe, i)
    flat = topk_ref_rows(index_ref.score(qc[:, :D], qs, bc[:, :D], bs), k)
    got = ivf_ref.search(q, x, centroids, k, nlist)
    assert (got[0] == flat[0]).all() and (bits(got[1]) == bits(flat[1])).all()       # every list probed: the flat lists


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def trained():
    x = synth_descriptors(6, 3000, 200)
    return x, ivf_ref.train(x, 16, iters=10, seed=0)


def test_fixture_lists_are_uneven_and_some_query_runs_short(trained):
    """x = synth_descriptors(6, 3000, 200), nlist = 16: a list of more than 256 rows (two tiles of the scan) and one of
    fewer than 64; with q = synth_descriptors(5, 33, 200) and nprobe = 1 some query has fewer than 100 candidates (a
    short row at k = 100)."""
    x, centroids = trained
    lens = np.diff(ivf_ref.build(x, centroids)['list_off'])
    print('list sizes %d .. %d' % (lens.min(), lens.max()))
    assert lens.sum() == 3000 and lens.max() > 256 and lens.min() < 64
    q = synth_descriptors(5, 33, 200)
    cand = lens[ivf_ref.probe(*index_ref.quantize(q), centroids, 1)[:, 0]]
    print('smallest candidate set %d' % cand.min())
    assert cand.min() < 100
    idx, vals = ivf_ref.search(q, x, centroids, 100, 1)
    assert (idx[cand < 100, -1] == -1).all() and np.isnan(vals[cand < 100, -1]).all() and (idx[cand >= 100] >= 0).all()


def test_restatement_training_closes_nine_tenths_of_the_gap(trained):
    """The mean exact cosine of a row to its centroid: the quantised-assignment fp32 training gains at least nine tenths of
    what an fp64 Lloyd run with exact assignments gains from the same initial centroids."""
    x, centroids = trained
    sample, first = ivf_ref.train_sample(x, 16, 0)
    start = ivf_ref.objective(x, x[first], (x.astype(np.float64) @ x[first].astype(np.float64).T).argmax(axis=1))
    c64, l64 = ivf_ref.lloyd64(x, first, 10)
    best = ivf_ref.objective(x, c64, l64)
    got = ivf_ref.objective(x, centroids, ivf_ref.assign(*index_ref.quantize(x), centroids))
    print('objective %.5f -> %.5f, fp64 Lloyd %.5f' % (start, got, best))
    assert best > start and got - start >= 0.9 * (best - start)


def test_training_argument_errors():
    x = synth_descriptors(6, 40, 16)
    with pytest.raises(ValueError):
        ivf_ref.train(x[:7], 8)
    bad = x.copy()
    bad[3, 2] = np.inf
    with pytest.raises(ValueError):
        ivf_ref.train(bad, 8)
    a, b = ivf_ref.train(x, 8, iters=3), ivf_ref.train(x, 8, iters=3, max_rows=4000)
    assert (bits(a) == bits(b)).all()
    sample, first = ivf_ref.train_sample(x, 8, seed=0, max_rows=20)
    assert len(sample) == 20 and (np.diff(first) > 0).all() and first.max() < 20

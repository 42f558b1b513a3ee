"""The inverted-file int8 index on the device (dir_segment_sums, dir_ivf_scan_i8, index.IVFInt8Index, python -m
dirtorch_amd.retrieve --index ivf).  The quantised score is one defined fp32 number, so the scan is compared bit for bit
with tests/index_ref.py, a search over every list with Int8Index.search, and a search over fewer lists with the numpy
restatement of tests/ivf_ref.py on the device-trained centroids; only the sums of a training step have a bound, the one
include/dir_engine.h states."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import index_ref
import ivf_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- segment_sums ------------------------------------------------------------------------------------------------------
SEG_LENS = [0, 1, 37, 0, 300, 5, 64, 17, 0]       # empty segments (first, inner, last), one row, more rows than a pass of 16


def _segments(r, N):
    """(order, seg_off): SEG_LENS rows each, drawn from a permutation of the N rows (not every row is used)"""
    seg_off = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int32)
    return r.permutation(N)[:seg_off[-1]].astype(np.int32), seg_off


def _seg_ref(x, order, seg_off):
    """fp64 sums and sums of |x| of every segment"""
    x = x.astype(np.float64)
    s = np.stack([x[order[a:b]].sum(axis=0) for a, b in zip(seg_off[:-1], seg_off[1:])])
    m = np.stack([np.abs(x[order[a:b]]).sum(axis=0) for a, b in zip(seg_off[:-1], seg_off[1:])])
    return s, m


@pytest.mark.parametrize('D', [1, 63, 200, 2048])
def test_segment_sums_exact_on_small_integers(D):
    """Operands in [-3, 3]: every partial sum is an integer below 2^24, exact in fp32 in any order.  Contiguous rows, rows
    at a pitch of D + 3 (scalar loads) and D + 4, and the sums at a pitch through the C ABI."""
    from dirtorch_amd import _lib, ops
    r = np.random.RandomState(160 + D)
    N = 500
    x = r.randint(-3, 4, (N, D)).astype(np.float32)
    order, seg_off = _segments(r, N)
    want = _seg_ref(x, order, seg_off)[0].astype(np.float32)
    got = ops.segment_sums(_cuda(x), _cuda(order, np.int32), _cuda(seg_off, np.int32))
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(SEG_LENS), D)
    assert (got.cpu().numpy() == want).all()
    assert not got[[0, 3, 8]].any()
    for pitch in (3, 4):
        wide = torch.full((N, D + pitch), float('nan'), device='cuda')
        wide[:, :D] = _cuda(x)
        assert (ops.segment_sums(wide[:, :D], _cuda(order, np.int32), _cuda(seg_off, np.int32)).cpu().numpy() == want).all()
    out = torch.full((len(SEG_LENS), D + 6), -7.0, device='cuda')
    dx, do, ds = _cuda(x), _cuda(order, np.int32), _cuda(seg_off, np.int32)
    _lib.call('dir_segment_sums', _lib.ptr(dx), D, N, D, _lib.ptr(do), _lib.ptr(ds), len(SEG_LENS), _lib.ptr(out), D + 6,
              _lib.stream_ptr())
    assert (out[:, :D].cpu().numpy() == want).all() and (out[:, D:] == -7).all()


@pytest.mark.parametrize('D', [200, 2048])
def test_segment_sums_within_the_stated_bound_and_reproducible(D):
    """|sum - fp64 sum| <= n_s 2^-24 sum |x| (include/dir_engine.h); two calls give the same bits."""
    from dirtorch_amd import ops
    r = np.random.RandomState(170)
    N = 500
    x = (r.standard_normal((N, D)) * np.exp(r.uniform(-3, 3, (N, 1)))).astype(np.float32)
    order, seg_off = _segments(r, N)
    want, mass = _seg_ref(x, order, seg_off)
    args = (_cuda(x), _cuda(order, np.int32), _cuda(seg_off, np.int32))
    got = ops.segment_sums(*args)
    again = ops.segment_sums(*args)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    bound = np.array(SEG_LENS, np.float64)[:, None] * 2.0 ** -24 * mass
    print('D = %d: max error %.3g of its bound' % (D, (err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all()


# ---- ivf_scan ----------------------------------------------------------------------------------------------------------
LENS = [0, 1, 255, 256, 257, 0, 700, 31, 300]      # a tile of the scan is 256 rows: one short of it, one, one and a row, three
NLIST, NROWS = len(LENS), sum(LENS)
LIST_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
GAP, PAST, FILL = 2, 7, 12345                      # empty columns between slots, columns past the width, what they hold


def _codes(r, n, D, junk=False):
    """asymmetric random codes [n, ldc] over the whole range -127 .. 127; junk: the padding bytes hold noise"""
    c = np.zeros((n, index_ref.pad64(D)), np.int8)
    if junk:
        c[:] = r.randint(-127, 128, c.shape)
    c[:, :D] = r.randint(-127, 128, (n, D))
    return c


def _check_scan(dev, D, want, ids, probe):
    """One ops.ivf_scan call on the table `probe` [Q, nprobe] (slots GAP columns apart, in a buffer PAST columns wider than
    the stated width) against the flat scores `want` [Q, NROWS]: ids of every column, score bits of every covered one."""
    from dirtorch_amd import ops
    Q, nprobe = probe.shape
    plen = np.where(probe >= 0, np.array(LENS)[np.maximum(probe, 0)], 0)
    col_off = (np.cumsum(plen + GAP, axis=1) - plen - GAP).astype(np.int32)
    width = int((col_off + plen).max()) + 3
    exp_ids = np.full((Q, width), -1, np.int32)
    exp_scores = np.zeros((Q, width), np.float32)
    covered = np.zeros((Q, width), bool)
    for q in range(Q):
        for p in range(nprobe):
            l = probe[q, p]
            if l >= 0:
                cols, rows = slice(col_off[q, p], col_off[q, p] + LENS[l]), slice(LIST_OFF[l], LIST_OFF[l + 1])
                exp_ids[q, cols], exp_scores[q, cols], covered[q, cols] = ids[rows], want[q, rows], True
    scores = torch.full((Q, width + PAST), float(FILL), dtype=torch.float32, device='cuda')
    out_ids = torch.full((Q, width + PAST), FILL, dtype=torch.int32, device='cuda')
    dq, dsq, db, dsb, dids, doff = dev
    got_s, got_i = ops.ivf_scan(dq[:Q], dsq[:Q], db, dsb, dids, doff, _cuda(probe, np.int32), _cuda(col_off, np.int32),
                                D, width=width, out=(scores, out_ids))
    assert got_s.data_ptr() == scores.data_ptr() and tuple(got_s.shape) == (Q, width) == tuple(got_i.shape)
    gi, gs = out_ids.cpu().numpy(), scores.cpu().numpy()
    assert (gi[:, :width] == exp_ids).all(), np.argwhere(gi[:, :width] != exp_ids)[:5]
    ok = (bits(gs[:, :width]) == bits(exp_scores)) | (np.isnan(gs[:, :width]) & np.isnan(exp_scores))
    assert ok[covered].all(), np.argwhere(~ok & covered)[:5]
    assert (gi[:, width:] == FILL).all() and (gs[:, width:] == FILL).all()
    # without `out` and `width`: the call sizes the rows itself
    got_s, got_i = ops.ivf_scan(dq[:Q], dsq[:Q], db, dsb, dids, doff, _cuda(probe, np.int32), _cuda(col_off, np.int32), D)
    assert tuple(got_i.shape) == (Q, width - 3) and (got_i.cpu().numpy() == exp_ids[:, :width - 3]).all()
    # ... and with the probe tables prepared by the caller
    tables = ops.ivf_probe_tables(doff, _cuda(probe, np.int32), _cuda(col_off, np.int32))
    assert tables[5] == width - 3 and all(t.dtype == torch.int32 and t.is_cuda for t in tables[:4])
    again_s, again_i = ops.ivf_scan(dq[:Q], dsq[:Q], db, dsb, dids, doff, _cuda(probe, np.int32), _cuda(col_off, np.int32), D,
                                    tables=tables)
    assert torch.equal(again_i, got_i) and torch.equal(again_s.view(torch.int32)[again_i >= 0], got_s.view(torch.int32)[got_i >= 0])


@pytest.mark.parametrize('D', [1, 64, 65, 200, 320, 448, 640, 2048])
def test_ivf_scan_is_the_restatement(D):
    """Hand-made lists, no training: every covered column carries index_ref.score's bits and its row's id, every other
    column id -1, and nothing past the width is written.  Q = 1 / 33 / 97 / 200 queries with 1 / 3 / 9 distinct random
    lists each (-1 in some slots); 200 queries that all probe the 700-row list (seven groups of 32 per tile); a table
    that leaves lists out; one NaN scale on each side; noise in the padding of the database codes.  D = 448: four slabs,
    the last a half (the first re-issue of the four-stage ring), 640: five slabs (the ring wraps)."""
    r = np.random.RandomState(180 + D)
    cq, cb = _codes(r, 200, D), _codes(r, NROWS, D, junk=True)
    sq = np.exp(r.uniform(-8, 2, 200)).astype(np.float32)
    sb = np.exp(r.uniform(-8, 2, NROWS)).astype(np.float32)
    sb[5], sq[7] = np.nan, np.nan
    ids = r.permutation(NROWS).astype(np.int32)
    want = index_ref.score(cq[:, :D], sq, cb[:, :D], sb)
    dev = (_cuda(cq, np.int8), _cuda(sq), _cuda(cb, np.int8), _cuda(sb), _cuda(ids, np.int32), _cuda(LIST_OFF, np.int32))
    for Q in (1, 33, 97, 200):
        for nprobe in (1, 3, 9):
            probe = np.stack([r.permutation(NLIST)[:nprobe] for _ in range(Q)]).astype(np.int32)
            if nprobe > 1:
                probe[r.rand(Q, nprobe) < 0.15] = -1
            _check_scan(dev, D, want[:Q], ids, probe)
    _check_scan(dev, D, want, ids, np.full((200, 1), 6, np.int32))
    nobody = np.stack([r.permutation([0, 1, 3, 7, 8])[:3] for _ in range(40)]).astype(np.int32)      # lists 2, 4, 6: no query
    _check_scan(dev, D, want[:40], ids, nobody)
    _check_scan(dev, D, want[:5], ids, np.full((5, 2), -1, np.int32))                                   # no list at all


# ---- IVFInt8Index ------------------------------------------------------------------------------------------------------
NL = 16


@pytest.fixture(scope='module')
def sets():
    """The inputs tests/test_ivf_cpu.py checks the fixture conditions on, a device-trained index over them, the flat int8
    index of the same rows and the trained centroids on the host."""
    from dirtorch_amd.index import IVFInt8Index, Int8Index
    q, b = synth_descriptors(5, 33, 200), synth_descriptors(6, 3000, 200)
    ivf = IVFInt8Index(200, NL).train(b, iters=10, seed=0).add(b)
    return dict(q=q, b=b, ivf=ivf, flat=Int8Index(200).add(b), centroids=ivf.centroids.cpu().numpy())


def test_every_list_probed_gives_the_flat_index_lists(sets, tmp_path):
    q, b, ivf, flat = sets['q'], sets['b'], sets['ivf'], sets['flat']
    assert len(ivf) == 3000 and ivf.nlist == NL
    for k in (10, 100):
        want = flat.search(q, k)
        for kw in ({}, dict(scratch_bytes=8 * 3000 * 5)):
            idx, vals = ivf.search(q, k, nprobe=NL, **kw)
            assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
            _same((idx, vals), want, '%r, k = %d' % (kw, k))
    np.save(str(tmp_path / 'b.npy'), b)
    mm = np.load(str(tmp_path / 'b.npy'), mmap_mode='r')
    for k, R in ((10, 40), (100, 400)):
        want = flat.search(q, k, rerank=R, source=_cuda(b))
        for source in (_cuda(b), mm):
            _same(ivf.search(q, k, nprobe=NL, rerank=R, source=source, scratch_bytes=8 * 3000 * 7), want, 'rerank %d' % R)


def test_same_set_over_every_list(sets):
    from dirtorch_amd.index import IVFInt8Index, Int8Index
    b = sets['b'][:600]
    ivf, flat = IVFInt8Index(200, 8).train(b).add(b), Int8Index(200).add(b)
    for k, kw in ((20, {}), (20, dict(scratch_bytes=8 * 600 * 250)), (600, {})):
        idx, vals = ivf.search(b, k, nprobe=8, same_set=True, **kw)
        _same((idx, vals), flat.search(b, k, same_set=True), 'k = %d' % k)
        assert (idx.cpu().numpy() != np.arange(600)[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    _same(ivf.search(b, 20, nprobe=8, rerank=80, source=b, same_set=True), flat.search(b, 20, rerank=80, source=b, same_set=True))


def test_the_store_does_not_depend_on_the_add_calls(sets):
    """One call, three calls and three calls of mixed kinds (ndarray, CPU tensor, CUDA tensor) build the same list-major
    store, which is the restatement's on the device-trained centroids - ids ascending inside every list."""
    from dirtorch_amd.index import IVFInt8Index
    q, b, one = sets['q'], sets['b'], sets['ivf']
    want = ivf_ref.build(b, sets['centroids'])
    assert (one.ids.cpu().numpy() == want['ids']).all() and (one.list_off.cpu().numpy() == want['list_off']).all()
    assert (one.codes.cpu().numpy() == want['codes']).all() and (bits(one.scales.cpu().numpy()) == bits(want['scales'])).all()
    lens = np.diff(want['list_off'])
    assert lens.max() > 256 and lens.min() < 64
    for parts in ((b[:1000], b[1000:1001], b[1001:]),
                  (b[:1000], torch.from_numpy(b[1000:1001]), torch.from_numpy(b[1001:]).cuda())):
        index = IVFInt8Index(200, NL)
        index._set_centroids(one.centroids.clone())
        for part in parts:
            index.add(part)
        assert len(index) == 3000
        for name in ('codes', 'ids', 'list_off'):
            assert torch.equal(getattr(index, name), getattr(one, name)), name
        assert torch.equal(index.scales.view(torch.int32), one.scales.view(torch.int32))
        _same(index.search(q, 10, nprobe=NL), sets['flat'].search(q, 10))
        _same(index.search(q, 10, nprobe=2), one.search(q, 10, nprobe=2))


@pytest.mark.parametrize('nprobe', [1, 2, 4])
def test_probed_search_is_the_restatement(sets, nprobe):
    """Given the centroids the whole search is defined: the lists equal ivf_ref's masked search, ids and value bits,
    including the rows that run short at k = 100, nprobe = 1."""
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    for k in (10, 100):
        want = ivf_ref.search(q, b, sets['centroids'], k, nprobe)
        for kw in ({}, dict(scratch_bytes=8 * 400 * 5)):
            _same(ivf.search(q, k, nprobe=nprobe, **kw), want, 'k = %d, %r' % (k, kw))
    if nprobe == 1:
        assert (want[0][:, -1] == -1).any() and (want[0][:, 0] >= 0).all()
    own = np.arange(33, dtype=np.int32) * 7
    qq = b[own]                                                          # queries that ARE rows: exclude leaves them out
    idx = ivf.search(qq, 10, nprobe=nprobe)[0].cpu().numpy()
    want = ivf_ref.search(qq, b, sets['centroids'], 10, nprobe)
    assert (idx == want[0]).all()


def test_search_pads_a_chunk_whose_rows_all_run_short():
    """Forty rows in four hand-set lists of 10, 4, 14 and 12 (no training), k = 40: with one list probed a query has 4 - 14
    neighbours, with two 14 - 26, so every chunk of queries is narrower than k and search widens it with empty columns
    before the top-k.  The lists equal ivf_ref's, ids and value bits with their (-1, NaN) tails, in one chunk and in
    chunks of two queries."""
    from dirtorch_amd.index import IVFInt8Index
    b, q = synth_descriptors(6, 3000, 200)[:40], synth_descriptors(5, 33, 200)[:5]
    c = b[[0, 10, 20, 30]]
    index = IVFInt8Index(200, 4)
    index._set_centroids(_cuda(c))
    index.add(b)
    assert index._lens.tolist() == [10, 4, 14, 12] == np.diff(ivf_ref.build(b, c)['list_off']).tolist()
    for nprobe, least, most in ((1, 4, 14), (2, 14, 26)):
        want = ivf_ref.search(q, b, c, 40, nprobe)
        found = (want[0] >= 0).sum(axis=1)
        assert found.min() == least and found.max() == most and most < 40         # every query runs short
        assert (want[0][:, most:] == -1).all() and np.isnan(want[1][:, most:]).all()
        for kw in ({}, dict(scratch_bytes=8 * 40 * 2)):                             # 8 bytes a column, 40 columns: two queries
            _same(index.search(q, 40, nprobe=nprobe, **kw), want, 'nprobe = %d, %r' % (nprobe, kw))


def test_rerank_over_probed_lists(sets):
    """rerank = R over two lists: the restatement's R best, re-scored by ops.gather_scores and ranked again; a host source
    gives the CUDA source's result bit for bit."""
    from dirtorch_amd import ops
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    k, R = 10, 40
    cand = _cuda(ivf_ref.search(q, b, sets['centroids'], R, 2)[0], np.int32)
    want = ops.topk(ops.gather_scores(_cuda(q), _cuda(b), cand), k, ids=cand)
    got = ivf.search(q, k, nprobe=2, rerank=R, source=_cuda(b))
    _same(got, want)
    _same(ivf.search(q, k, nprobe=2, rerank=R, source=b, scratch_bytes=8 * 400 * 5), got)


def test_training_is_reproducible_and_closes_nine_tenths_of_the_gap(sets):
    """train twice: identical bits.  The mean exact cosine of a row to its centroid gains at least nine tenths of what an
    fp64 Lloyd run with exact assignments gains from the same initial centroids (tests/test_ivf_cpu.py holds the
    restatement to the same condition)."""
    from dirtorch_amd.index import IVFInt8Index
    b, ivf = sets['b'], sets['ivf']
    again = IVFInt8Index(200, NL).train(_cuda(b), iters=10, seed=0)
    assert torch.equal(again.centroids.view(torch.int32), ivf.centroids.view(torch.int32))
    assert torch.equal(again.ccodes, ivf.ccodes) and torch.equal(again.cscales.view(torch.int32), ivf.cscales.view(torch.int32))
    norms = np.linalg.norm(sets['centroids'].astype(np.float64), axis=1)
    assert np.abs(norms - 1).max() < 1e-5
    sample, first = ivf_ref.train_sample(b, NL, 0)
    start = ivf_ref.objective(b, b[first], (b.astype(np.float64) @ b[first].astype(np.float64).T).argmax(axis=1))
    c64, l64 = ivf_ref.lloyd64(b, first, 10)
    best = ivf_ref.objective(b, c64, l64)
    got = ivf_ref.objective(b, sets['centroids'], ivf_ref.assign(*index_ref.quantize(b), sets['centroids']))
    print('objective %.5f -> %.5f on the device, fp64 Lloyd %.5f' % (start, got, best))
    assert best > start and got - start >= 0.9 * (best - start)
    # a sample: more rows than max_rows
    small = IVFInt8Index(200, NL).train(b, iters=2, seed=3, max_rows=500)
    pick = np.sort(np.random.RandomState(3).choice(3000, 500, replace=False))
    same = IVFInt8Index(200, NL).train(b[pick], iters=2, seed=3)
    assert torch.equal(small.centroids.view(torch.int32), same.centroids.view(torch.int32))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd.index import IVFInt8Index
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    path = str(tmp_path / 'ivf.npz')
    ivf.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'centroids', 'codes', 'ids', 'list_off', 'nlist', 'scales']
        assert f['codes'].shape == (3000, 200) and f['codes'].dtype == np.int8 and f['centroids'].shape == (NL, 200)
        assert f['ids'].dtype == np.int32 and f['list_off'].dtype == np.int32 and f['list_off'].shape == (NL + 1,)
    back = IVFInt8Index.load(path)
    assert back.D == 200 and back.nlist == NL and len(back) == 3000
    for name in ('codes', 'ids', 'list_off', 'ccodes'):
        assert torch.equal(getattr(back, name), getattr(ivf, name)), name
    for name in ('scales', 'centroids', 'cscales'):
        assert torch.equal(getattr(back, name).view(torch.int32), getattr(ivf, name).view(torch.int32)), name
    for kw in (dict(nprobe=2), dict(nprobe=NL, rerank=40, source=_cuda(b))):
        _same(back.search(q, 10, **kw), ivf.search(q, 10, **kw))
    for nprobe in (0, NL + 1):
        with pytest.raises(ValueError):
            ivf.search(q, 10, nprobe=nprobe)
    fresh = IVFInt8Index(200, NL)
    with pytest.raises(ValueError):
        fresh.search(q, 10)                                      # before train
    with pytest.raises(ValueError):
        fresh.add(b)                                             # before train
    with pytest.raises(ValueError):
        fresh.train(b[:NL - 1])                                  # fewer rows than lists
    bad = b[:100].copy()
    bad[17, 3] = np.nan
    with pytest.raises(ValueError):
        fresh.train(bad)
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, rerank=40)                   # no source
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, rerank=9, source=b)          # R < k
    with pytest.raises(ValueError):
        ivf.search(q, 3001, nprobe=2)
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, same_set=True)
    with pytest.raises(ValueError):
        ivf.add(np.zeros((3, 199), np.float32))
    with pytest.raises(ValueError):
        IVFInt8Index(200, 0)


# ---- python -m dirtorch_amd.retrieve --index ivf -----------------------------------------------------------------------
def test_retrieve_cli_with_an_inverted_file(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): with every list probed (--nlist 8 --nprobe 8) the
    .npz of --index ivf equals that of --index int8 for the same inputs."""
    import dir_oracle as O
    r = np.random.RandomState(69)
    N, D, k = 120, 32, 7
    x = np.round(r.standard_normal((N, D)) * 4).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + key: v for key, v in sd.items()}}, str(tmp_path / 'ck.pt'))
    pkg = os.path.join(ROOT, 'deep-image-retrieval_amd')
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    runs = {'ivf': ['--index', 'ivf', '--nlist', '8', '--nprobe', '8', '--rerank', '28'], 'int8': ['--index', 'int8', '--rerank', '28']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', outs[name]] + flags, env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    got, want = np.load(outs['ivf']), np.load(outs['int8'])
    assert sorted(got.files) == ['idx', 'scores'] and got['idx'].dtype == np.int32 and got['scores'].dtype == np.float32
    _same((got['idx'], got['scores']), (want['idx'], want['scores']), 'ivf against int8')
    assert (got['idx'] != np.arange(N)[:, None]).all() and (got['idx'] >= 0).all()

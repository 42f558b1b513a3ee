"""The IVF-PQ index on the device (dir_ivfpq_base, dir_ivfpq_scan, index.IVFPQIndex, python -m dirtorch_amd.retrieve --index
ivfpq).  Residuals, coarse terms and scores are chains of single fp32 operations in a fixed order (include/dir_engine.h),
so - given the device's centroids and codebooks - everything is compared bit for bit with the numpy restatement of
tests/ivfpq_ref.py; the one exception is the reconstruction error of the trained index, a property with a stated bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ivfpq_ref
import pq_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits_ok(got, want):
    """bit for bit; where the reference holds a NaN, a NaN (an x86 host and the device give inf - inf different signs)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- ivfpq_base --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,M', [(8, 1), (12, 3), (64, 8), (2048, 64), (256, 128), (80, 2)])
def test_base_is_the_restatement(D, M):
    """nlist = 5, Q = 1 and 33, four slots: random lists, -1 in some slots, one row that probes one list in every slot;
    queries at a pitch; centroid 2 holds an infinity (its terms are +-inf or, against a zero, NaN) and query 4 is zero."""
    from dirtorch_amd import ops
    r = np.random.RandomState(500 + D + M)
    q = (r.standard_normal((33, D)) * np.exp(r.uniform(-2, 2, (33, 1)))).astype(np.float32)
    q[4] = 0
    c = r.standard_normal((5, D)).astype(np.float32)
    c[2, D // 2] = np.inf
    probe = r.randint(0, 5, (33, 4)).astype(np.int32)
    probe[r.rand(33, 4) < 0.2] = -1
    probe[0], probe[3], probe[4] = (2, -1, 0, 2), (1, 1, 1, 1), (2, 3, -1, 4)
    want = ivfpq_ref.base(q, c, M, probe=probe)
    assert np.isnan(want[probe < 0]).all() and np.isinf(want[0, 0]) and np.isnan(want[4, 0]) and not bits(want[4, 1]).any()
    dq, dc, dp = _cuda(q), _cuda(c), _cuda(probe, np.int32)
    for Q in (1, 33):
        got = ops.ivfpq_base(dq[:Q], dc, dp[:Q], M)
        assert got.dtype == torch.float32 and tuple(got.shape) == (Q, 4) and got.is_cuda
        ok = _bits_ok(got.cpu().numpy(), want[:Q])
        assert ok.all(), (Q, np.argwhere(~ok)[:5])
    wide = torch.full((33, D + 5), float('nan'), device='cuda')
    wide[:, :D] = dq
    cwide = torch.full((5, D + 3), float('nan'), device='cuda')
    cwide[:, :D] = dc
    assert _bits_ok(ops.ivfpq_base(wide[:, :D], cwide[:, :D], dp, M).cpu().numpy(), want).all()
    assert tuple(ops.ivfpq_base(dq, dc, dp[:, :0], M).shape) == (33, 0)
    for bad in (lambda: ops.ivfpq_base(dq, dc[:, :D - 1], dp, M), lambda: ops.ivfpq_base(dq, dc, dp[:5], M),
                lambda: ops.ivfpq_base(dq, dc, dp, D + 1), lambda: ops.ivfpq_base(dq, dc, dp, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.ivfpq_base(dq, dc, dp.long(), M)


# ---- ivfpq_scan --------------------------------------------------------------------------------------------------------
T = 1024                                           # the columns (rows of a list) a workgroup of the scan owns
LENS = [0, 1, T - 1, T, T + 1, 2 * T + 3, 37]      # an empty list, one row, a workgroup less / exactly / plus one, two and three
NLIST, NROWS = len(LENS), sum(LENS)
LIST_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
GAP, PAST, FILL = 2, 7, 12345                      # empty columns between slots, columns past the width, what they hold
SQ = 33


def _scan_case(M, r):
    """(tables [33, M, 256], codes [NROWS, ldc + 4] with noise in the padding): tables over a wide range of magnitudes with
    -0.0, +-inf and NaN entries (some scores are +-inf, some NaN); query 1 has every entry -0.0"""
    t = (r.standard_normal((SQ, M, 256)) * np.exp(r.uniform(-6, 6, (SQ, M, 1)))).astype(np.float32)
    flat = t.reshape(-1)
    n = flat.size
    flat[r.randint(0, n, n // 50)] = -0.0
    flat[r.randint(0, n, max(n // 3000, 3))] = np.inf
    flat[r.randint(0, n, max(n // 3000, 3))] = -np.inf
    flat[r.randint(0, n, max(n // 5000, 2))] = np.nan
    t[1] = -0.0
    codes = r.randint(0, 256, (NROWS, (M + 3) // 4 * 4 + 4)).astype(np.uint8)
    return t, codes


def _expected(t, codes, M, ids, probe, base, col_off, width):
    """ids, score bits and the covered columns of one call, slot by slot through ivfpq_ref.scan"""
    Q, nprobe = probe.shape
    exp_ids = np.full((Q, width), -1, np.int32)
    exp_scores = np.zeros((Q, width), np.float32)
    covered = np.zeros((Q, width), bool)
    for p in range(nprobe):
        for l in range(NLIST):
            qs = np.flatnonzero(probe[:, p] == l)
            if not len(qs) or not LENS[l]:
                continue
            rows = slice(LIST_OFF[l], LIST_OFF[l + 1])
            s = ivfpq_ref.scan(t[qs], np.repeat(base[qs, p:p + 1], LENS[l], axis=1), codes[rows, :M])
            for j, q in enumerate(qs):
                n = max(0, min(LENS[l], width - col_off[q, p]))                  # a slot stores nothing at or past width
                cols = slice(col_off[q, p], col_off[q, p] + n)
                exp_ids[q, cols], exp_scores[q, cols], covered[q, cols] = ids[rows][:n], s[j, :n], True
    return exp_ids, exp_scores, covered


def _check_scan(dev, t, codes, M, ids, probe, base, cut=0):
    """One ops.ivfpq_scan call on the table `probe` [Q, nprobe] (slots GAP columns apart, in a buffer PAST columns wider than
    the stated width; cut > 0: a width that many columns short of the last slot's end): ids of every column below the
    width, score bits of every covered one, the fill value past it; then the call that sizes its own rows."""
    from dirtorch_amd import ops
    dt, dc, dids, doff = dev
    Q, nprobe = probe.shape
    plen = np.where(probe >= 0, np.array(LENS)[np.maximum(probe, 0)], 0)
    col_off = (np.cumsum(plen + GAP, axis=1) - plen - GAP).astype(np.int32)
    reach = int((col_off + plen).max())
    width = reach - cut if cut else reach + 3
    exp_ids, exp_scores, covered = _expected(t, codes, M, ids, probe, base, col_off, width)
    scores = torch.full((Q, width + PAST), float(FILL), dtype=torch.float32, device='cuda')
    out_ids = torch.full((Q, width + PAST), FILL, dtype=torch.int32, device='cuda')
    args = (dt[:Q], _cuda(base), dc, dids, doff, _cuda(probe, np.int32), _cuda(col_off, np.int32))
    got_s, got_i = ops.ivfpq_scan(*args, width=width, out=(scores, out_ids))
    assert got_s.data_ptr() == scores.data_ptr() and tuple(got_s.shape) == (Q, width) == tuple(got_i.shape)
    gi, gs = out_ids.cpu().numpy(), scores.cpu().numpy()
    assert (gi[:, :width] == exp_ids).all(), np.argwhere(gi[:, :width] != exp_ids)[:5]
    ok = _bits_ok(gs[:, :width], exp_scores)
    assert ok[covered].all(), np.argwhere(~ok & covered)[:5]
    assert (gi[:, width:] == FILL).all() and (gs[:, width:] == FILL).all()
    if not cut:                                                               # without `out` and `width`
        auto_s, auto_i = ops.ivfpq_scan(*args)
        assert tuple(auto_i.shape) == (Q, reach) and (auto_i.cpu().numpy() == exp_ids[:, :reach]).all()
        assert _bits_ok(auto_s.cpu().numpy(), exp_scores[:, :reach])[covered[:, :reach]].all()
        again_s, again_i = ops.ivfpq_scan(*args)                              # two calls: the same bits
        assert torch.equal(again_i, auto_i)
        assert torch.equal(again_s.view(torch.int32)[again_i >= 0], auto_s.view(torch.int32)[auto_i >= 0])
    return gs[:, :width], covered


# the issue's M; the kernel changes form at 8 | 9 .. 16 | 17 .. 32 | 33 .. 64 | 65 .. 128 code bytes, and pads an odd number
# of code words (M = 1, 3, 9, 17, 33, 65) with tables of -0.0
@pytest.mark.parametrize('M', [1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128])
def test_scan_is_the_restatement(M):
    """Hand-made lists, no training.  Q = 1, 2, 3, 33 with nprobe = 1, 3 and nlist distinct random lists each (-1 in some
    slots); base entries of -0.0 and NaN; noise in the padding bytes of the codes; a width that cuts the last slot; a table
    of empty slots only."""
    r = np.random.RandomState(600 + M)
    t, codes = _scan_case(M, r)
    ids = r.permutation(NROWS).astype(np.int32)
    dev = (_cuda(t), _cuda(codes, np.uint8), _cuda(ids, np.int32), _cuda(LIST_OFF, np.int32))
    seen_nan = seen_inf = False
    for Q in (1, 2, 3, SQ):
        for nprobe in (1, 3, NLIST):
            probe = np.stack([r.permutation(NLIST)[:nprobe] for _ in range(Q)]).astype(np.int32)
            if nprobe > 1:
                probe[r.rand(Q, nprobe) < 0.15] = -1
            base = (r.standard_normal((Q, nprobe)) * 3).astype(np.float32)
            base[r.rand(Q, nprobe) < 0.2] = -0.0
            base[r.rand(Q, nprobe) < 0.1] = np.nan
            gs, covered = _check_scan(dev, t, codes, M, ids, probe, base)
            seen_nan, seen_inf = seen_nan or np.isnan(gs[covered]).any(), seen_inf or np.isinf(gs[covered]).any()
    assert seen_nan and seen_inf
    # query 1, every table entry -0.0, from a base of -0.0: the score is -0.0; from +0.0: +0.0
    probe = np.array([[5, 4], [5, 4]], np.int32)
    base = np.array([[1, 2], [-0.0, 0.0]], np.float32)
    gs, covered = _check_scan(dev, t, codes, M, ids, probe, base)
    assert (bits(gs[1, :LENS[5]]) == 0x80000000).all() and not bits(gs[1, LENS[5] + GAP:LENS[5] + GAP + LENS[4]]).any()
    # the width cuts the last slot (list 5, three workgroups) 1500 columns short; nothing at or past it is written
    _check_scan(dev, t, codes, M, ids, np.array([[3, 5], [4, 5], [6, 5]], np.int32), r.standard_normal((3, 2)).astype(np.float32),
                cut=1500)
    _check_scan(dev, t, codes, M, ids, np.full((2, 3), -1, np.int32), np.zeros((2, 3), np.float32))      # no list at all
    _check_scan(dev, t, codes, M, ids, np.array([[0, 1]], np.int32), np.ones((1, 2), np.float32))        # an empty list, one row


def test_scan_wrapper_argument_errors_and_unpitched_codes():
    from dirtorch_amd import ops
    assert ops.ivfpq_scan_cols() == T                                  # the list lengths above are cut around it
    r = np.random.RandomState(690)
    M = 6
    t, codes = _scan_case(M, r)
    ids = np.arange(NROWS, dtype=np.int32)
    dt, dids, doff = _cuda(t[:2]), _cuda(ids, np.int32), _cuda(LIST_OFF, np.int32)
    probe, col_off, base = _cuda([[6, 1], [1, 6]], np.int32), _cuda([[0, 40], [0, 3]], np.int32), _cuda([[1, 2], [3, 4]])
    want_s, want_i = ops.ivfpq_scan(dt, base, _cuda(codes, np.uint8), dids, doff, probe, col_off)
    assert tuple(want_s.shape) == (2, 41)
    got_s, got_i = ops.ivfpq_scan(dt, base, _cuda(codes[:, :M], np.uint8), dids, doff, probe, col_off)   # ldc = 6: copied to 8
    assert torch.equal(got_i, want_i) and torch.equal(got_s.view(torch.int32)[got_i >= 0], want_s.view(torch.int32)[want_i >= 0])
    dc = _cuda(codes, np.uint8)
    with pytest.raises(ValueError):
        ops.ivfpq_scan(dt, base, dc[:, :M - 1], dids, doff, probe, col_off)
    with pytest.raises(ValueError):
        ops.ivfpq_scan(dt, base, dc, dids[:-1], doff, probe, col_off)
    with pytest.raises(ValueError):
        ops.ivfpq_scan(dt, base[:, :1], dc, dids, doff, probe, col_off)
    with pytest.raises(ValueError):
        ops.ivfpq_scan(dt, base, dc, dids, doff, probe[:1], col_off)
    with pytest.raises(TypeError):
        ops.ivfpq_scan(dt, base, dc, dids, doff, probe.long(), col_off)
    with pytest.raises(TypeError):
        ops.ivfpq_scan(dt, base, dc.to(torch.int8), dids, doff, probe, col_off)
    with pytest.raises(ValueError):
        ops.ivfpq_scan(dt, base, dc, dids, doff, probe, col_off, width=41,
                       out=(torch.empty(2, 40, device='cuda'), torch.empty(2, 40, dtype=torch.int32, device='cuda')))


# ---- IVFPQIndex --------------------------------------------------------------------------------------------------------
PD, PM, NL = 64, 8, 16


@pytest.fixture(scope='module')
def sets():
    """33 queries, 3000 clustered rows of 64 values, an index of 16 lists and 8 sub-spaces trained on the rows; its centroids
    and codebooks on the host, the restatement's store and its flat score matrix (every list below is a top-k of it)."""
    from dirtorch_amd.index import IVFPQIndex
    q, b = synth_descriptors(5, 33, PD), synth_descriptors(6, 3000, PD)
    index = IVFPQIndex(PD, NL, PM).train(b, iters=10, seed=0).add(b)
    c, cb = index.centroids.cpu().numpy(), index.codebooks.cpu().numpy()
    return dict(q=q, b=b, index=index, c=c, cb=cb, store=ivfpq_ref.build(b, c, cb), flat=ivfpq_ref.flat_scores(q, b, c, cb))


def test_store_is_the_restatement(sets):
    index, store = sets['index'], sets['store']
    assert len(index) == 3000 and index.M == PM and index.nlist == NL and index.nbytes() == 3000 * (PM + 4)
    assert tuple(index.codes.shape) == (3000, PM) and index.codes.dtype == torch.uint8
    assert (index.ids.cpu().numpy() == store['ids']).all() and (index.list_off.cpu().numpy() == store['list_off']).all()
    assert (index.codes.cpu().numpy()[:, :PM] == store['codes']).all()
    assert (index._lens == np.diff(store['list_off'])).all()


@pytest.mark.parametrize('nprobe', [1, 2, 4, 16])
def test_search_is_the_restatement(sets, nprobe):
    q, b, index = sets['q'], sets['b'], sets['index']
    for k in (1, 10, 100):
        want = ivfpq_ref.search(q, b, sets['c'], sets['cb'], k, nprobe, flat=sets['flat'])
        idx, vals = index.search(q, k, nprobe=nprobe)
        assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
        _same((idx, vals), want, 'k = %d' % k)
        # three chunks of 11 queries: 8 bytes per column of the nprobe longest lists and 1024 * M bytes of tables each
        width = max(int(np.sort(index._lens)[-nprobe:].sum()), k)
        _same(index.search(_cuda(q), k, nprobe=nprobe, scratch_bytes=11 * (8 * width + 1024 * PM)), want, 'chunks, k = %d' % k)


def test_the_store_does_not_depend_on_the_add_calls(sets):
    from dirtorch_amd.index import IVFPQIndex
    q, b, one = sets['q'], sets['b'], sets['index']
    for parts in ((b[:1000], b[1000:1001], b[1001:]),
                  (b[:1000], torch.from_numpy(b[1000:1001]), torch.from_numpy(b[1001:]).cuda())):
        index = IVFPQIndex(PD, NL, PM)
        index._set_centroids(one.centroids.clone())
        index.codebooks = one.codebooks.clone()
        for part in parts:
            index.add(part)
        assert len(index) == 3000
        for name in ('codes', 'ids', 'list_off'):
            assert torch.equal(getattr(index, name), getattr(one, name)), name
        for nprobe in (2, NL):
            _same(index.search(q, 10, nprobe=nprobe), one.search(q, 10, nprobe=nprobe))


def test_same_set_and_short_rows(sets):
    """600 rows that are their own queries, nprobe = 1, k one above the smallest list: the rows of that list have fewer than
    k neighbours and end in (-1, NaN); no query is in its own list."""
    from dirtorch_amd.index import IVFPQIndex
    b = sets['b'][:600]
    index = IVFPQIndex(PD, 8, PM).train(b, iters=2).add(b)
    c, cb = index.centroids.cpu().numpy(), index.codebooks.cpu().numpy()
    own = np.arange(600, dtype=np.int32)
    lens = index._lens[index._lens > 0]
    flat = ivfpq_ref.flat_scores(b, b, c, cb)
    for k, nprobe in ((int(lens.min()) + 1, 1), (20, 3), (600, 8)):
        idx, vals = index.search(b, k, nprobe=nprobe, same_set=True)
        _same((idx, vals), ivfpq_ref.search(b, b, c, cb, k, nprobe, exclude=own, flat=flat), 'k = %d, nprobe = %d' % (k, nprobe))
        assert (idx.cpu().numpy() != own[:, None]).all()
        if nprobe == 1:
            assert (idx[:, -1] == -1).any() and (idx[:, 0] >= 0).any()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N, every list: a row has N - 1 neighbours


def test_rerank_with_a_device_and_a_host_source(sets, tmp_path):
    """rerank = R over two lists: the restatement's R best, re-scored by ops.gather_scores against the fp32 rows and ranked
    again; a host ndarray and a memmap give the CUDA source's result bit for bit."""
    from dirtorch_amd import ops
    q, b, index = sets['q'], sets['b'], sets['index']
    np.save(str(tmp_path / 'b.npy'), b)
    mm = np.load(str(tmp_path / 'b.npy'), mmap_mode='r')
    for k, R in ((10, 40), (100, 130)):
        cand = _cuda(ivfpq_ref.search(q, b, sets['c'], sets['cb'], R, 2, flat=sets['flat'])[0], np.int32)
        want = ops.topk(ops.gather_scores(_cuda(q), _cuda(b), cand), k, ids=cand)
        _same(index.search(q, k, nprobe=2, rerank=R, source=_cuda(b)), want, 'device source, R = %d' % R)
        _same(index.search(q, k, nprobe=2, rerank=R, source=b, scratch_bytes=8 * 1200 * 11), want, 'host source')
        _same(index.search(q, k, nprobe=2, rerank=R, source=mm), want, 'memmap source')


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd.index import IVFPQIndex
    q, b, index = sets['q'], sets['b'], sets['index']
    path = str(tmp_path / 'ivfpq.npz')
    index.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'M', 'centroids', 'codebooks', 'codes', 'ids', 'list_off', 'nlist']
        assert f['codes'].shape == (3000, PM) and f['codes'].dtype == np.uint8 and f['centroids'].shape == (NL, PD)
        assert f['codebooks'].shape == (PM, 256, PD // PM) and f['codebooks'].dtype == np.float32
        assert f['ids'].dtype == np.int32 and f['list_off'].dtype == np.int32 and f['list_off'].shape == (NL + 1,)
        saved = {name: f[name] for name in f.files}
    back = IVFPQIndex.load(path)
    assert back.D == PD and back.nlist == NL and back.M == PM and len(back) == 3000
    for name in ('codes', 'ids', 'list_off', 'ccodes'):
        assert torch.equal(getattr(back, name), getattr(index, name)), name
    for name in ('centroids', 'cscales', 'codebooks'):
        assert torch.equal(getattr(back, name).view(torch.int32), getattr(index, name).view(torch.int32)), name
    for kw in (dict(nprobe=2), dict(nprobe=NL, rerank=40, source=_cuda(b))):
        _same(back.search(q, 10, **kw), index.search(q, 10, **kw))
    off = saved['list_off'].copy()
    off[3] = off[-1] + 5                                             # not ascending
    for bad in (dict(codes=saved['codes'].astype(np.int8)), dict(codes=saved['codes'][:, :PM - 1]), dict(ids=saved['ids'][:-1]),
                dict(codebooks=saved['codebooks'][:, :255]), dict(codebooks=saved['codebooks'][:PM - 1]), dict(M=np.int64(7)),
                dict(centroids=saved['centroids'][:-1]), dict(list_off=saved['list_off'][:-1]), dict(list_off=off),
                dict(list_off=saved['list_off'] + 1), dict(nlist=np.int64(0))):
        np.savez(str(tmp_path / 'bad.npz'), **dict(saved, **bad))
        with pytest.raises(ValueError):
            IVFPQIndex.load(str(tmp_path / 'bad.npz'))
    for D, nlist, M in ((64, 16, 0), (64, 16, 7), (64, 16, 129), (0, 16, 1), (64, 0, 8), (64, 65536, 8)):
        with pytest.raises(ValueError):
            IVFPQIndex(D, nlist, M)
    fresh = IVFPQIndex(PD, NL, PM)
    for call in (lambda: fresh.search(q, 10), lambda: fresh.add(b), lambda: fresh.save(path),      # before train
                 lambda: fresh.train(b[:255]),                       # fewer rows than the 256 centroids of a sub-space
                 lambda: IVFPQIndex(PD, 300, PM).train(b[:299]),     # fewer rows than lists
                 lambda: fresh.train(b, max_rows=100),
                 lambda: index.train(b),                             # after add
                 lambda: index.search(q, 10, nprobe=0), lambda: index.search(q, 10, nprobe=NL + 1),
                 lambda: index.search(q, 10, nprobe=2, rerank=40),   # no source
                 lambda: index.search(q, 10, nprobe=2, rerank=9, source=b),
                 lambda: index.search(q, 10, nprobe=2, rerank=40, source=b[:100]),
                 lambda: index.search(q, 3001, nprobe=2), lambda: index.search(q, 0, nprobe=2),
                 lambda: index.search(q, 10, nprobe=2, same_set=True),
                 lambda: index.search(q[:, :63], 10), lambda: index.add(np.zeros((3, 63), np.float32))):
        with pytest.raises(ValueError):
            call()
    bad = b[:300].copy()
    bad[17, 3] = np.inf
    with pytest.raises(ValueError):
        fresh.train(bad)
    idx, vals = index.search(q[:0], 10)
    assert tuple(idx.shape) == (0, 10) and tuple(vals.shape) == (0, 10)
    assert len(index.add(b[:0])) == 3000


def test_training_is_reproducible_shares_the_coarse_quantiser_and_reduces_the_error(sets):
    """Two runs from one seed: identical bits, from host rows and from device rows.  The centroids are IVFInt8Index.train's
    for the same rows and seed, bit for bit, so a row lands in the same list in both indexes.  A sample (more rows than
    max_rows) is the sorted RandomState choice.  The mean squared reconstruction error of the residuals (fp64 on the host,
    from the stored codes) is below 0.9 of that of a PQIndex(64, 8) trained on the same rows with the same iterations and
    seed: the numpy restatement gives 0.80 (tests/test_ivfpq_cpu.py), the device's fixed-order sums differ from numpy's in
    last bits so the trajectories may part, and 0.9 leaves half the gap."""
    from dirtorch_amd import ops
    from dirtorch_amd.index import IVFInt8Index, IVFPQIndex, PQIndex
    b, index, store = sets['b'], sets['index'], sets['store']
    again = IVFPQIndex(PD, NL, PM).train(_cuda(b), iters=10, seed=0)
    assert torch.equal(again.centroids.view(torch.int32), index.centroids.view(torch.int32))
    assert torch.equal(again.codebooks.view(torch.int32), index.codebooks.view(torch.int32))
    ivf = IVFInt8Index(PD, NL).train(b, iters=10, seed=0).add(b)
    assert torch.equal(ivf.centroids.view(torch.int32), index.centroids.view(torch.int32))
    assert torch.equal(ivf.ids, index.ids) and torch.equal(ivf.list_off, index.list_off)
    small = IVFPQIndex(PD, NL, PM).train(b, iters=2, seed=3, max_rows=500)
    pick = np.sort(np.random.RandomState(3).choice(3000, 500, replace=False))
    same = IVFPQIndex(PD, NL, PM).train(b[pick], iters=2, seed=3)
    assert torch.equal(small.centroids.view(torch.int32), same.centroids.view(torch.int32))
    assert torch.equal(small.codebooks.view(torch.int32), same.codebooks.view(torch.int32))
    res = ivfpq_ref.residuals(b, sets['c'], store['lists'])[store['ids']]     # list-major, as the codes are stored
    err_res = pq_ref.reconstruction_error(res, sets['cb'], index.codes.cpu().numpy()[:, :PM])
    flat = PQIndex(PD, PM).train(b, iters=10, seed=0)
    codes = ops.pq_encode(_cuda(b), flat.codebooks).cpu().numpy()[:, :PM]
    err_flat = pq_ref.reconstruction_error(b, flat.codebooks.cpu().numpy(), codes)
    print('reconstruction error %.6f residual, %.6f flat: ratio %.4f' % (err_res, err_flat, err_res / err_flat))
    assert np.isfinite([err_res, err_flat]).all() and err_res < 0.9 * err_flat


# ---- python -m dirtorch_amd.retrieve --index ivfpq ---------------------------------------------------------------------
def test_retrieve_cli_with_ivfpq(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): the .npz of --index ivfpq --nlist 4 --nprobe 2
    --pq-m 8, without and with --rerank, equals IVFPQIndex.search on the same descriptors; an M that does not divide the
    width ends the run, and so do missing --nlist / --pq-m before anything is loaded."""
    import dir_oracle as O
    from dirtorch_amd import retrieve
    from dirtorch_amd.index import IVFPQIndex
    r = np.random.RandomState(73)
    N, D, k = 300, 32, 7
    x = np.round(r.standard_normal((N, D)) * 4).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + key: v for key, v in sd.items()}}, str(tmp_path / 'ck.pt'))
    pkg = os.path.join(ROOT, 'deep-image-retrieval_amd')
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = ['--dataset', 'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
            str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0', '--topk', str(k)]
    flags = ['--index', 'ivfpq', '--nlist', '4', '--nprobe', '2']
    runs = {'raw': flags + ['--pq-m', '8'], 'rerank': flags + ['--pq-m', '8', '--rerank', '28'], 'odd': flags + ['--pq-m', '5']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = {name: subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve'] + base + ['--output', outs[name]] + f,
                                    env=env) for name, f in runs.items()}
    codes = {name: p.wait(timeout=300) for name, p in procs.items()}
    assert codes['raw'] == 0 and codes['rerank'] == 0 and codes['odd'] != 0 and not os.path.exists(outs['odd'])
    index = IVFPQIndex(D, 4, 8).train(x).add(x)
    for name, kw in (('raw', {}), ('rerank', dict(rerank=28, source=x))):
        got = np.load(outs[name])
        assert sorted(got.files) == ['idx', 'scores'] and got['idx'].dtype == np.int32 and got['scores'].dtype == np.float32
        _same((got['idx'], got['scores']), index.search(x, k, nprobe=2, same_set=True, **kw), name)
        assert (got['idx'] != np.arange(N)[:, None]).all()
    with pytest.raises(SystemExit, match='pq-m'):
        retrieve.main(base + ['--output', outs['odd'], '--index', 'ivfpq', '--nlist', '4'])
    with pytest.raises(SystemExit, match='nlist'):
        retrieve.main(base + ['--output', outs['odd'], '--index', 'ivfpq', '--pq-m', '8'])

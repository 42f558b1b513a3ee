"""The device planner of the inverted files on the device (dir_ivf_plan, ops.ivf_plan, search(plan=)).  Everything is an
integer table or a list that must not change, so every comparison is exact: the planned tables with the numpy restatement
(tests/ivf_plan_ref.py) AND with what the host path makes (index._InvertedLists._slots' col_off, ops.ivf_probe_tables); the
two scans on planned tables, the host width and an over-sized grid with the same scans on the host tables; a search with
plan='device' with the same search with plan='host'; and a search with plan='device' under torch's synchronisation check."""
import numpy as np
import pytest
import torch

import ivf_plan_ref
from index_util import cuda as _cuda
from synth import synth_descriptors

pytestmark = pytest.mark.gpu

KEYS = ('pair_off', 'pair_q', 'pair_col', 'item_off')


def _host_tables(list_off, probe):
    """what a search with plan='host' makes: col_off as index._InvertedLists._slots does (an empty slot: length 0), the rest
    from ops.ivf_probe_tables"""
    from dirtorch_amd import ops
    lens = list_off[1:] - list_off[:-1]
    lens = torch.where(probe >= 0, lens[probe.long().clamp(min=0)], lens.new_zeros(()))
    col_off = torch.cumsum(lens, dim=1, dtype=torch.int32) - lens
    return col_off, ops.ivf_probe_tables(list_off, probe, col_off)


def _check_tables(probe, list_off):
    """ops.ivf_plan on (probe, list_off) ndarrays: every output equals the restatement's and the host path's; returns the
    planned (col_off, tables, counts)"""
    from dirtorch_amd import ops
    dprobe, doff = _cuda(probe, np.int32), _cuda(list_off, np.int32)
    want = ivf_plan_ref.plan(probe, list_off)
    bound = int(want['counts'][0]) + 5
    col_off, tables, counts = ops.ivf_plan(doff, dprobe, bound)
    assert col_off.dtype == torch.int32 and tuple(col_off.shape) == probe.shape and col_off.is_cuda
    assert len(tables) == 6 and tables[4] == bound and tables[5] is None
    assert torch.equal(col_off.cpu(), torch.from_numpy(want['col_off'])), 'col_off against the restatement'
    for key, got in zip(KEYS, tables):
        assert got.dtype == torch.int32 and got.is_cuda, key
        assert torch.equal(got.cpu(), torch.from_numpy(want[key])), key + ' against the restatement'
    assert torch.equal(counts.cpu(), torch.from_numpy(want['counts'])), (counts.cpu(), want['counts'])
    host_col, host = _host_tables(doff, dprobe)
    assert torch.equal(col_off, host_col), 'col_off against the host path'
    for key, got, ref in zip(KEYS, tables, host):
        assert torch.equal(got, ref), key + ' against ops.ivf_probe_tables'
    assert counts.tolist() == [host[4], host[5]]
    return col_off, tables, counts


def _distinct(r, Q, nprobe, nlist):
    return np.stack([r.permutation(nlist)[:nprobe] for _ in range(Q)]).astype(np.int32)


def _offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


EDGE_LENS = [0, 1, 255, 256, 257, 5000]


def _case(name):
    r = np.random.RandomState(sum(map(ord, name)))
    if name == 'one':
        return np.zeros((1, 1), np.int32), _offsets([5])
    if name == 'one_query_8_of_64':
        return _distinct(r, 1, 8, 64), _offsets(r.choice(EDGE_LENS, 64))
    if name == '70x32_of_1024':
        return _distinct(r, 70, 32, 1024), _offsets(r.choice(EDGE_LENS, 1024, p=[.1, .1, .2, .2, .2, .2]))
    if name == 'empty_trailing_lists':
        return _distinct(r, 9, 6, 20), _offsets(list(r.choice(EDGE_LENS[1:], 15)) + [0] * 5)
    if name == 'unprobed_trailing_lists':
        return _distinct(r, 9, 6, 12), _offsets(r.choice(EDGE_LENS, 20))
    if name == 'empty_slots':
        probe = _distinct(r, 12, 7, 30)
        probe[:, 3] = -1                      # in the middle of every row
        probe[::2, 6] = -1                    # at the end of every other
        probe[5] = -1                         # a whole row
        return probe, _offsets(r.choice(EDGE_LENS, 30))
    if name in ('33_share_a_list', '100_share_a_list'):          # 2 and 4 groups of 32 pairs on the list's 3 tiles
        Q = int(name.split('_')[0])
        return np.full((Q, 1), 2, np.int32), _offsets([10, 0, 700, 300])
    if name == '65535_lists':
        return _distinct(r, 2, 16, 65535), _offsets(r.choice(EDGE_LENS, 65535, p=[.3, .3, .1, .1, .1, .1]))
    if name == 'pair_limit':
        from dirtorch_amd import ops
        assert ops.ivf_plan_max_pairs() % 32 == 0
        return _distinct(r, ops.ivf_plan_max_pairs() // 32, 32, 1024), _offsets(r.choice(EDGE_LENS[:5], 1024))
    raise KeyError(name)


CASES = ['one', 'one_query_8_of_64', '70x32_of_1024', 'empty_trailing_lists', 'unprobed_trailing_lists', 'empty_slots',
         '33_share_a_list', '100_share_a_list', '65535_lists', 'pair_limit']


@pytest.mark.parametrize('name', CASES)
def test_planned_tables_are_the_restatement_and_the_host_tables(name):
    probe, list_off = _case(name)
    _, tables, counts = _check_tables(probe, list_off)
    if name.endswith('share_a_list'):
        groups = {'33': 2, '100': 4}[name.split('_')[0]]
        assert counts[0].item() == 3 * groups and tables[3].tolist() == [0, 0, 0, 3 * groups, 3 * groups]
    if name == 'pair_limit':
        from dirtorch_amd import ops
        assert probe.size == ops.ivf_plan_max_pairs()


def test_two_calls_give_equal_tables():
    from dirtorch_amd import ops
    probe, list_off = _case('70x32_of_1024')
    dprobe, doff = _cuda(probe, np.int32), _cuda(list_off, np.int32)
    a, b = ops.ivf_plan(doff, dprobe, 100000), ops.ivf_plan(doff, dprobe, 100000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and a[0].data_ptr() != b[0].data_ptr()
    assert all(torch.equal(x, y) for x, y in zip(a[1][:4], b[1][:4]))


def test_a_pair_past_the_limit_is_refused_and_nothing_is_written():
    from dirtorch_amd import _lib, ops
    limit = ops.ivf_plan_max_pairs()
    doff = _cuda(_offsets([3, 4]), np.int32)
    probe = torch.zeros(limit + 1, 1, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='cut the queries'):
        ops.ivf_plan(doff, probe, 10)
    with pytest.raises(ValueError, match='65535'):
        ops.ivf_plan(torch.zeros(65537, dtype=torch.int32, device='cuda'), probe[:2], 10)
    with pytest.raises(ValueError, match='items_bound'):
        ops.ivf_plan(doff, probe[:2], ops.ivf_scan_max_items() + 1)
    with pytest.raises(TypeError):
        ops.ivf_plan(doff.long(), probe[:2], 10)
    with pytest.raises(TypeError):
        ops.ivf_plan(doff, probe[:2].long(), 10)
    with pytest.raises(ValueError):
        ops.ivf_plan(doff, probe[:2, 0], 10)
    with pytest.raises(ValueError):
        ops.ivf_plan(doff[:1], probe[:2], 10)
    # the entry itself: DIR_ERR_INVALID, and none of the six outputs is touched
    outs = [torch.full((limit + 8,), 77, dtype=torch.int32, device='cuda') for _ in range(6)]
    rc = _lib.load().dir_ivf_plan(_lib.ptr(probe), limit + 1, 1, _lib.ptr(doff), 2, *[_lib.ptr(t) for t in outs], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and b'dir_ivf_plan_max_pairs' in _lib.load().dir_last_error()
    assert all((t == 77).all().item() for t in outs)
    # ... and at the limit it is taken
    col_off, _, counts = ops.ivf_plan(doff, probe[:limit], limit)
    assert counts.tolist() == [limit // 32, 3] and not col_off.any().item()
    # no query: nothing launched, empty tables
    col_off, tables, counts = ops.ivf_plan(doff, probe[:0], 0)
    assert tuple(col_off.shape) == (0, 1) and counts.tolist() == [0, 0] and tables[0].tolist() == [0, 0, 0] == tables[3].tolist()


# ---- the two scans on planned tables ---------------------------------------------------------------------------------------
LENS = [0, 1, 255, 256, 257, 0, 700, 31, 300]      # a tile of the scan is 256 rows: one short of it, one, one and a row, three


def _scan_probes():
    r = np.random.RandomState(77)
    some = _distinct(r, 70, 3, len(LENS))
    some[r.rand(70, 3) < 0.15] = -1
    return [('70 queries at 3 lists, empty slots', some), ('one query at every list', _distinct(r, 1, len(LENS), len(LENS))),
            ('100 queries share the 700-row list', np.full((100, 1), 6, np.int32))]


@pytest.mark.parametrize('D', [64, 200])
@pytest.mark.parametrize('kind', ['i8', 'fp4'])
def test_scans_on_planned_tables_equal_the_scans_on_host_tables(kind, D):
    """Planned tables, the width a search takes (the nprobe longest lists) and a grid several times the true workgroup
    count: out_ids equal everywhere, the score bits wherever a column is covered."""
    from dirtorch_amd import ops
    N = sum(LENS)
    x, xq = _cuda(synth_descriptors(31, N, D)), _cuda(synth_descriptors(32, 100, D))
    ids = _cuda(np.random.RandomState(5).permutation(N), np.int32)
    doff = _cuda(_offsets(LENS), np.int32)
    db, dq = (ops.quantize_rows(x), ops.quantize_rows(xq)) if kind == 'i8' else (ops.quantize_rows_fp4(x), ops.quantize_rows_fp4(xq))
    scan = ops.ivf_scan if kind == 'i8' else ops.ivf_scan_fp4
    for what, probe in _scan_probes():
        Q, nprobe = probe.shape
        dprobe = _cuda(probe, np.int32)
        width = int(np.sort(LENS)[-nprobe:].sum())
        host_col, host = _host_tables(doff, dprobe)
        assert 0 < host[4] <= ivf_plan_ref.items_bound(LENS, Q, nprobe) and host[5] <= width
        bound = 4 * host[4] + 7
        col_off, tables, _ = ops.ivf_plan(doff, dprobe, bound)
        qargs = [t[:Q] for t in dq]
        want_s, want_i = scan(*qargs, *db, ids, doff, dprobe, host_col, D, width=width, tables=host)
        got_s, got_i = scan(*qargs, *db, ids, doff, dprobe, col_off, D, width=width, tables=tables)
        assert tuple(got_i.shape) == (Q, width) and (want_i >= 0).any().item(), what
        assert torch.equal(got_i, want_i), what
        assert torch.equal(got_s.view(torch.int32)[got_i >= 0], want_s.view(torch.int32)[want_i >= 0]), what
        with pytest.raises(ValueError, match='explicit width'):
            scan(*qargs, *db, ids, doff, dprobe, col_off, D, tables=tables)


# ---- search(plan=) ---------------------------------------------------------------------------------------------------------
NL = 16


@pytest.fixture(scope='module')
def sets():
    """3000 clustered rows in 16 trained lists (uneven: tests/test_ivf_cpu.py checks a list above 256 rows and one below 64),
    in the int8 and in the fp4 inverted file - one training, the same centroids - and 600 rows in 8 lists for same_set"""
    from dirtorch_amd.index import IVFFp4Index, IVFInt8Index
    b = synth_descriptors(6, 3000, 200)
    i8 = IVFInt8Index(200, NL).train(b, iters=10, seed=0).add(b)
    fp4 = IVFFp4Index(200, NL)
    fp4._set_centroids(i8.centroids.clone())
    fp4.add(b)
    small8 = IVFInt8Index(200, 8).train(b[:600]).add(b[:600])
    small4 = IVFFp4Index(200, 8)
    small4._set_centroids(small8.centroids.clone())
    small4.add(b[:600])
    return dict(q=_cuda(synth_descriptors(5, 70, 200)), b=b, db=_cuda(b), i8=i8, fp4=fp4, small_i8=small8, small_fp4=small4)


def _same_lists(got, want, what):
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[0].shape == want[0].shape, what
    assert torch.equal(got[0], want[0]), (what, (got[0] != want[0]).nonzero()[:5])
    same = (got[1].view(torch.int32) == want[1].view(torch.int32)) | (torch.isnan(got[1]) & torch.isnan(want[1]))
    assert same.all().item(), (what, (~same).nonzero()[:5])


def _both(index, q, k, what, **kw):
    host = index.search(q, k, plan='host', **kw)
    _same_lists(index.search(q, k, plan='device', **kw), host, what + ', device')
    _same_lists(index.search(q, k, plan='auto', **kw), host, what + ', auto')
    return host


@pytest.mark.parametrize('kind', ['i8', 'fp4'])
def test_search_with_the_device_plan_returns_the_host_plan_lists(sets, kind):
    from dirtorch_amd import ops
    index, q = sets[kind], sets['q']
    for Q in (1, 70):
        for nprobe in (1, 4, NL):
            _both(index, q[:Q], 10, 'Q %d nprobe %d' % (Q, nprobe), nprobe=nprobe)
    # k above the candidates of one list: (-1, NaN) tails
    idx, vals = _both(index, q, 400, 'k above the candidates', nprobe=1)
    assert (idx[:, -1] == -1).any().item() and torch.isnan(vals[idx == -1]).all().item() and (idx[:, 0] >= 0).all().item()
    # a re-rank against the fp32 rows on the device
    _both(index, q, 100, 'rerank', nprobe=4, rerank=400, source=sets['db'])
    # three chunks of queries
    width = max(int(np.sort(index._lens)[-4:].sum()), 10)
    per_query = 8 * width + (0 if kind == 'i8' else sum(ops.fp4_widths(200)) + 4)
    _both(index, q, 10, 'three chunks', nprobe=4, scratch_bytes=30 * per_query)
    # every slot of every chunk is planned by its own call: chunks of one query
    _both(index, q[:5], 10, 'chunks of one', nprobe=2, scratch_bytes=1)
    # the queries are the database
    small, rows = sets['small_' + kind], sets['db'][:600]
    idx, _ = _both(small, rows, 20, 'same_set', nprobe=3, same_set=True)
    assert (idx.cpu() != torch.arange(600)[:, None]).all().item()
    _both(small, rows, 20, 'same_set, rerank', nprobe=3, same_set=True, rerank=80, source=rows)
    with pytest.raises(ValueError, match='plan'):
        index.search(q, 10, plan='gpu')


@pytest.mark.parametrize('kind', ['i8', 'fp4'])
def test_a_chunk_over_the_pair_limit_falls_back_or_raises(sets, kind):
    """1100 queries at all 16 lists are 17600 pairs in one chunk: 'auto' takes the host path and returns its lists, 'device'
    says why it cannot; cut into chunks of 500 queries (8000 pairs) both plan on the device."""
    from dirtorch_amd import ops
    index, q = sets[kind], sets['db'][:1100]
    assert 1100 * NL > ops.ivf_plan_max_pairs() >= 500 * NL
    host = index.search(q, 10, nprobe=NL, plan='host')
    _same_lists(index.search(q, 10, nprobe=NL, plan='auto'), host, 'auto')
    with pytest.raises(ValueError, match='pairs'):
        index.search(q, 10, nprobe=NL, plan='device')
    per_query = 8 * 3000 + (0 if kind == 'i8' else sum(ops.fp4_widths(200)) + 4)
    _same_lists(index.search(q, 10, nprobe=NL, plan='device', scratch_bytes=500 * per_query), host, 'chunks of 500')


def test_ivfpq_takes_the_argument_and_stays_as_it_is(sets):
    """IVFPQIndex walks no inverted table and never synchronised: plan= is checked and changes nothing."""
    from dirtorch_amd.index import IVFPQIndex
    b = sets['b']
    index = IVFPQIndex(200, NL, 20).train(b, iters=3).add(b)
    host = index.search(sets['q'], 10, nprobe=4, plan='host')
    for plan in ('device', 'auto'):
        _same_lists(index.search(sets['q'], 10, nprobe=4, plan=plan), host, plan)
    with pytest.raises(ValueError, match='plan'):
        index.search(sets['q'], 10, plan='gpu')


# ---- no synchronisation ----------------------------------------------------------------------------------------------------
@pytest.fixture
def sync_is_an_error():
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(before)


@pytest.mark.parametrize('kind', ['i8', 'fp4'])
def test_search_with_the_device_plan_never_waits_for_the_host(sets, kind, sync_is_an_error):
    """Under torch.cuda.set_sync_debug_mode('error') a synchronising torch call raises.  First that the mode works on this
    build (an .item() raises); then search(plan='device') with queries - and a rerank source - on the device returns, in
    one chunk and in three, while the same call with plan='host' raises at ops.ivf_probe_tables' read-back."""
    index, q, db = sets[kind], sets['q'], sets['db']
    with pytest.raises(RuntimeError):
        q[0, 0].item()
    for kw in (dict(nprobe=4), dict(nprobe=4, rerank=40, source=db), dict(nprobe=1), dict(nprobe=4, scratch_bytes=300000)):
        got = index.search(q, 10, plan='device', **kw)
        with pytest.raises(RuntimeError):
            index.search(q, 10, plan='host', **kw)
        torch.cuda.set_sync_debug_mode('default')
        _same_lists(got, index.search(q, 10, plan='host', **kw), repr(sorted(kw)))
        torch.cuda.set_sync_debug_mode('error')

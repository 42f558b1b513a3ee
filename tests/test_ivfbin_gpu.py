"""The inverted file over sign-bit rows on the device (dir_code_sums, dir_ivf_scan_bin, index.IVFBinaryIndex, python -m
dirtorch_amd.retrieve --index ivfbin).  A score is dir_similarity_bin's number - an exact int32 times two fp32 factors -
whatever the cut of the work, so every comparison is on bits: the scan with tests/bin_ref.py's scores, a search over every
list with BinaryIndex.search, a search over fewer lists and the list-major store with the numpy restatement of
tests/ivfbin_ref.py on the device-trained centroids."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bin_ref
import ivfbin_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8(a):
    return _cuda(a, np.uint8)


def _i8(a):
    return _cuda(a, np.int8)


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- code_sums, ivf_scan_bin -------------------------------------------------------------------------------------------
LENS = [0, 1, 255, 256, 257, 0, 700, 31, 300]      # a tile of the scan is 256 rows: one short of it, one, one and a row, three
NLIST, NROWS = len(LENS), sum(LENS)
LIST_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
GAP, PAST, FILL = 2, 7, 12345                      # empty columns between slots, columns past the width, what they hold


def _queries(r, n, D):
    """int8 query rows [n, pad64(D) + 64]: codes below D, zero in D .. pad64(D) as the contract asks, and noise in the 64
    bytes past that, which the scan must not read"""
    pad = (D + 63) // 64 * 64
    qc = r.randint(-127, 128, (n, pad + 64)).astype(np.int8)
    qc[:, D:pad] = 0
    return qc


def _check_scan(dev, D, want, ids, probe):
    """One ops.ivf_scan_bin call on the table `probe` [Q, nprobe] (slots GAP columns apart, in a buffer PAST columns wider
    than the stated width) against the flat scores `want` [Q, NROWS]: ids of every column, score bits of every covered one;
    then the call that sizes its rows itself (width=None) and the call on caller-made tables and sums."""
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
    dprobe, dcol = _cuda(probe, np.int32), _cuda(col_off, np.int32)
    got_s, got_i = ops.ivf_scan_bin(dq[:Q], dsq[:Q], db, dsb, dids, doff, dprobe, dcol, D, width=width, out=(scores, out_ids))
    assert got_s.data_ptr() == scores.data_ptr() and tuple(got_s.shape) == (Q, width) == tuple(got_i.shape)
    gi, gs = out_ids.cpu().numpy(), scores.cpu().numpy()
    assert (gi[:, :width] == exp_ids).all(), np.argwhere(gi[:, :width] != exp_ids)[:5]
    ok = _bits_equal(gs[:, :width], exp_scores)
    assert ok[covered].all(), np.argwhere(~ok & covered)[:5]
    assert (gi[:, width:] == FILL).all() and (gs[:, width:] == FILL).all()
    # without `out` and `width`: the call sizes the rows itself
    got_s, got_i = ops.ivf_scan_bin(dq[:Q], dsq[:Q], db, dsb, dids, doff, dprobe, dcol, D)
    assert tuple(got_i.shape) == (Q, width - 3) and (got_i.cpu().numpy() == exp_ids[:, :width - 3]).all()
    ok = _bits_equal(got_s.cpu().numpy(), exp_scores[:, :width - 3])
    assert ok[covered[:, :width - 3]].all()
    # ... and with the probe tables and the query sums prepared by the caller
    tables = ops.ivf_probe_tables(doff, dprobe, dcol)
    assert tables[5] == width - 3 and all(t.dtype == torch.int32 and t.is_cuda for t in tables[:4])
    again_s, again_i = ops.ivf_scan_bin(dq[:Q], dsq[:Q], db, dsb, dids, doff, dprobe, dcol, D, tables=tables,
                                        qsums=ops.code_sums(dq[:Q], D))
    assert torch.equal(again_i, got_i) and torch.equal(again_s.view(torch.int32)[again_i >= 0], got_s.view(torch.int32)[got_i >= 0])


@pytest.mark.parametrize('D', [1, 64, 200, 1000, 1024, 1088, 2048, 2176, 3200, 4224])
def test_ivf_scan_bin_is_the_restatement(D):
    """Hand-made lists, no training: every covered column carries bin_ref.score's bits and its row's id, every other column
    id -1, and nothing past the width is written.  Q = 1 / 33 / 97 / 200 queries with 1 / 3 / 9 distinct random lists each
    (-1 in some slots); 200 queries that all probe the 700-row list (seven groups of 32 per tile); a table that leaves
    lists out; no list at all; one NaN and one zero scale on each side; the database bits past D are noise; the query rows
    are zero in D .. pad64(D) and noise in the 64 bytes past that (ldq = pad64(D) + 64), so a loader that reads past
    pad64(D) fails.  D = 1, 64, 200, 1000: one slab of 1024 k cut to 1, 1, 2, 8 chunks with a partial last sub-slab; 1024:
    one whole slab; 1088: a slab and one chunk; 2048: two slabs, no slot used twice; 2176: three slabs, the ring's first
    wrap; 3200 and 4224: four and five slabs, both parities of the wrap."""
    from dirtorch_amd import ops
    r = np.random.RandomState(330 + D)
    qc = _queries(r, 200, D)
    rows = r.randint(0, 256, (NROWS, bin_ref.width(D))).astype(np.uint8)
    sq = np.exp(r.uniform(-8, 2, 200)).astype(np.float32)
    sb = np.exp(r.uniform(-8, 2, NROWS)).astype(np.float32)
    sb[5], sb[9], sq[7], sq[11] = np.nan, 0, np.nan, 0
    sq[0] = 1.5                                         # (Q = 1 has a plain query)
    ids = r.permutation(NROWS).astype(np.int32)
    want = bin_ref.score(qc, sq, rows, sb, D)
    dev = (_i8(qc), _cuda(sq), _u8(rows), _cuda(sb), _cuda(ids, np.int32), _cuda(LIST_OFF, np.int32))
    sums = ops.code_sums(dev[0], D)
    assert sums.dtype == torch.int32 and (sums.cpu().numpy() == qc[:, :D].astype(np.int64).sum(axis=1)).all()
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


@pytest.mark.parametrize('D', [1152, 2048])
def test_scan_layout_one_hot_pairs(D):
    """tests/test_bin_gpu.py's one-hot walk through the list scan: query i is one-hot at k = i; row j of a single list holds
    the single bit k' = (a j + s) mod D, once with (a, s) = (1, 0) and once with (7, 3); all D queries probe the list, so
    every group row, tile row and k position is met (D = 1152: a whole slab and one chunk; 2048: two slabs).  t = +code
    where k == k', -code elsewhere: a wrong bit-to-byte order, chunk, sub-image, lane half or slab moves the positive cell."""
    from dirtorch_amd import ops
    i = np.arange(D)
    code = (1 + i % 127) * np.where(i % 3 == 1, -1, 1)
    qc = np.zeros((D, D), np.int8)
    qc[i, i] = code
    one = torch.ones(D, dtype=torch.float32, device='cuda')
    dq = _i8(qc)
    ids = _cuda(i, np.int32)
    list_off = _cuda(np.array([0, D]), np.int32)
    probe = torch.zeros(D, 1, dtype=torch.int32, device='cuda')
    for a, s in ((1, 0), (7, 3)):
        kb = (a * i + s) % D
        rows = np.zeros((D, bin_ref.width(D)), np.uint8)
        rows[i, kb >> 3] = 1 << (kb & 7)
        got_s, got_i = ops.ivf_scan_bin(dq, one, _u8(rows), one, ids, list_off, probe, probe, D)
        assert tuple(got_s.shape) == (D, D) and (got_i.cpu().numpy() == i[None, :]).all()
        got = got_s.cpu().numpy()
        hit = i[:, None] == kb[None, :]
        want = np.where(hit, code[:, None], -code[:, None]).astype(np.float32)
        assert (got == want).all(), (a, s, np.argwhere(got != want)[:5])
        assert (bits(got) == bits(bin_ref.score(qc, np.ones(D), rows, np.ones(D), D))).all()


def test_the_sum_is_exact_up_to_the_bound():
    """D = 131072, the widest row (128 slabs).  Every query code +-127 against rows of all ones, all zeros and alternating
    bits: |t| = 127 * D = 16 646 144 needs all 24 bits of the fp32 it becomes, and the kernel's 2 * acc passes through 2^25
    in int32.  Two lists, of 3 and of 40 rows, five queries that probe both."""
    from dirtorch_amd import ops
    D = bin_ref.MAX_DIM
    r = np.random.RandomState(340)
    Q, N = 5, 43
    qc = np.full((Q, D), 127, np.int8)
    qc[1, 1::2] = -127
    qc[2] = -127
    qc[3, 0::2] = -127
    qc[4] = np.where(r.rand(D) < 0.5, 127, -127)
    rows = r.randint(0, 256, (N, bin_ref.width(D))).astype(np.uint8)
    rows[0], rows[1], rows[2], rows[3], rows[4] = 0xff, 0, 0x55, 0xaa, 0xff
    rows[42] = 0xff
    t = bin_ref.dot(qc, rows, D)
    assert t[0, 0] == 127 * D == 16646144 and t[0, 1] == -127 * D and t[0, 2] == 0 and t[1, 2] == 127 * D and t[1, 3] == -127 * D
    assert t[2, 42] == -127 * D and t[0, 42] == 127 * D
    list_off = np.array([0, 3, 43], np.int32)
    probe = np.tile(np.array([[1, 0]], np.int32), (Q, 1))
    col_off = np.tile(np.array([[0, 40]], np.int32), (Q, 1))
    ids = r.permutation(N).astype(np.int32)
    order = np.concatenate([np.arange(3, 43), np.arange(3)])
    dev = (_u8(rows), _cuda(ids, np.int32), _cuda(list_off, np.int32), _cuda(probe, np.int32), _cuda(col_off, np.int32))
    one = np.ones(N, np.float32)
    got_s, got_i = ops.ivf_scan_bin(_i8(qc), _cuda(one[:Q]), dev[0], _cuda(one), *dev[1:], D)
    assert tuple(got_s.shape) == (Q, 43) and (got_i.cpu().numpy() == ids[order][None, :]).all()
    got = got_s.cpu().numpy()
    assert (got.astype(np.int64) == t[:, order]).all(), np.argwhere(got.astype(np.int64) != t[:, order])[:5]
    sq, sb = np.exp2(r.randint(-30, 30, Q)).astype(np.float32), r.uniform(0.5, 2, N).astype(np.float32)
    got_s, got_i = ops.ivf_scan_bin(_i8(qc), _cuda(sq), dev[0], _cuda(sb), *dev[1:], D)
    assert (bits(got_s.cpu().numpy()) == bits(bin_ref.score(qc, sq, rows, sb, D)[:, order])).all()


# ---- IVFBinaryIndex ----------------------------------------------------------------------------------------------------
NL = 16


@pytest.fixture(scope='module')
def sets():
    """bin_ref.rerank_sets() - the inputs tests/test_ivfbin_cpu.py checks the fixture conditions on - a device-trained index
    over them, the flat binary index of the same rows and the trained centroids on the host."""
    from dirtorch_amd.index import BinaryIndex, IVFBinaryIndex
    q, b = bin_ref.rerank_sets()
    ivf = IVFBinaryIndex(200, NL).train(b, iters=10, seed=0).add(b)
    return dict(q=q, b=b, ivf=ivf, flat=BinaryIndex(200).add(b), centroids=ivf.centroids.cpu().numpy())


def test_every_list_probed_gives_the_flat_binary_index_lists(sets, tmp_path):
    from dirtorch_amd.index import IVFInt8Index
    q, b, ivf, flat = sets['q'], sets['b'], sets['ivf'], sets['flat']
    assert len(ivf) == 3000 and ivf.nlist == NL and ivf.nbytes() == 3000 * (32 + 4 + 4)
    i8 = IVFInt8Index(200, NL).train(b, iters=10, seed=0)                 # the coarse side is the int8 inverted file's
    assert torch.equal(i8.centroids.view(torch.int32), ivf.centroids.view(torch.int32)) and torch.equal(i8.ccodes, ivf.ccodes)
    for k in (10, 100):
        want = flat.search(q, k)
        _same(want, bin_ref.search(q, b, k))
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
    from dirtorch_amd.index import BinaryIndex, IVFBinaryIndex
    b = sets['b'][:600]
    ivf, flat = IVFBinaryIndex(200, 8).train(b).add(b), BinaryIndex(200).add(b)
    for k, kw in ((20, {}), (20, dict(scratch_bytes=8 * 600 * 250)), (600, {})):
        idx, vals = ivf.search(b, k, nprobe=8, same_set=True, **kw)
        _same((idx, vals), flat.search(b, k, same_set=True), 'k = %d' % k)
        assert (idx.cpu().numpy() != np.arange(600)[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    _same(ivf.search(b, 20, nprobe=8, rerank=80, source=b, same_set=True), flat.search(b, 20, rerank=80, source=b, same_set=True))


def test_the_store_is_the_restatements_and_does_not_depend_on_the_add_calls(sets):
    """One call, three calls and three calls of mixed kinds (ndarray, CPU tensor, CUDA tensor) build the same list-major
    store, which is the restatement's on the device-trained centroids - ids ascending inside every list."""
    from dirtorch_amd.index import IVFBinaryIndex
    q, b, one = sets['q'], sets['b'], sets['ivf']
    want = ivfbin_ref.build(b, sets['centroids'])
    assert (one.ids.cpu().numpy() == want['ids']).all() and (one.list_off.cpu().numpy() == want['list_off']).all()
    assert (one.codes.cpu().numpy() == want['codes']).all() and (bits(one.scales.cpu().numpy()) == bits(want['scales'])).all()
    lens = np.diff(want['list_off'])
    assert lens.max() > 256 and lens.min() < 64
    for parts in ((b[:1000], b[1000:1001], b[1001:]),
                  (b[:1000], torch.from_numpy(b[1000:1001]), torch.from_numpy(b[1001:]).cuda())):
        index = IVFBinaryIndex(200, NL)
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
    """Given the centroids the whole search is defined: the lists equal ivfbin_ref's masked search, ids and value bits,
    including the rows that run short at k = 100, nprobe = 1, and the queries that are rows."""
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    for k in (10, 100):
        want = ivfbin_ref.search(q, b, sets['centroids'], k, nprobe)
        for kw in ({}, dict(scratch_bytes=8 * 400 * 5)):
            _same(ivf.search(q, k, nprobe=nprobe, **kw), want, 'k = %d, %r' % (k, kw))
    if nprobe == 1:
        assert (want[0][:, -1] == -1).any() and (want[0][:, 0] >= 0).all()
    own = np.arange(33, dtype=np.int32) * 7
    qq = b[own]                                                          # queries that ARE rows
    _same(ivf.search(qq, 10, nprobe=nprobe), ivfbin_ref.search(qq, b, sets['centroids'], 10, nprobe))


def test_search_pads_a_chunk_whose_rows_all_run_short():
    """Forty rows in four hand-set lists of 10, 4, 14 and 12 (no training), k = 40: with one list probed a query has 4 - 14
    neighbours, with two 14 - 26, so every chunk of queries is narrower than k and search widens it with empty columns
    before the top-k.  The lists equal ivfbin_ref's, ids and value bits with their (-1, NaN) tails, in one chunk and in
    chunks of two queries."""
    from dirtorch_amd.index import IVFBinaryIndex
    b, q = synth_descriptors(6, 3000, 200)[:40], synth_descriptors(5, 33, 200)[:5]
    c = b[[0, 10, 20, 30]]
    index = IVFBinaryIndex(200, 4)
    index._set_centroids(_cuda(c))
    index.add(b)
    assert index._lens.tolist() == [10, 4, 14, 12] == np.diff(ivfbin_ref.build(b, c)['list_off']).tolist()
    for nprobe, least, most in ((1, 4, 14), (2, 14, 26)):
        want = ivfbin_ref.search(q, b, c, 40, nprobe)
        found = (want[0] >= 0).sum(axis=1)
        assert found.min() == least and found.max() == most and most < 40         # every query runs short
        assert (want[0][:, most:] == -1).all() and np.isnan(want[1][:, most:]).all()
        for kw in ({}, dict(scratch_bytes=2 * (8 * 40 + 4))):                       # two queries: 40 columns and their sums
            _same(index.search(q, 40, nprobe=nprobe, **kw), want, 'nprobe = %d, %r' % (nprobe, kw))


def test_the_device_plan_gives_the_host_plans_bits_and_never_waits(sets):
    """plan='device' returns plan='host''s lists; under torch.cuda.set_sync_debug_mode('error') it returns with queries and a
    rerank source on the device, in one chunk and in three, where the same call with plan='host' raises at
    ops.ivf_probe_tables' read-back."""
    ivf = sets['ivf']
    q, db = _cuda(sets['q']), _cuda(sets['b'])
    cases = (dict(nprobe=4), dict(nprobe=4, rerank=40, source=db), dict(nprobe=1), dict(nprobe=4, scratch_bytes=300000),
             dict(nprobe=NL))
    hosts = [ivf.search(q, 10, plan='host', **kw) for kw in cases]
    for kw, host in zip(cases, hosts):
        _same(ivf.search(q, 10, plan='auto', **kw), host, 'auto %r' % sorted(kw))
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            q[0, 0].item()                                               # the mode works on this build
        got = []
        for kw in cases:
            got.append(ivf.search(q, 10, plan='device', **kw))
            with pytest.raises(RuntimeError):
                ivf.search(q, 10, plan='host', **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    for kw, g, host in zip(cases, got, hosts):
        _same(g, host, 'device %r' % sorted(kw))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd import ops
    from dirtorch_amd.index import BinaryIndex, IVFBinaryIndex
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    path = str(tmp_path / 'ivfbin.npz')
    ivf.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'bits', 'centroids', 'ids', 'list_off', 'nlist', 'scales']
        assert f['bits'].shape == (3000, 25) and f['bits'].dtype == np.uint8 and f['scales'].shape == (3000,)
        assert f['centroids'].shape == (NL, 200) and f['ids'].dtype == np.int32 and f['list_off'].shape == (NL + 1,)
    back = IVFBinaryIndex.load(path)
    assert back.D == 200 and back.nlist == NL and len(back) == 3000 and back.nbytes() == ivf.nbytes()
    for name in ('codes', 'ids', 'list_off', 'ccodes'):
        assert torch.equal(getattr(back, name), getattr(ivf, name)), name
    for name in ('scales', 'centroids', 'cscales'):
        assert torch.equal(getattr(back, name).view(torch.int32), getattr(ivf, name).view(torch.int32)), name
    for kw in (dict(nprobe=2), dict(nprobe=NL, rerank=40, source=_cuda(b))):
        _same(back.search(q, 10, **kw), ivf.search(q, 10, **kw))
    # the sign-bit half of the file is BinaryIndex's format: the flat index reads the list-major rows as they lie
    flat = BinaryIndex.load(path)
    assert torch.equal(flat.codes, ivf.codes) and torch.equal(flat.scales.view(torch.int32), ivf.scales.view(torch.int32))
    with pytest.raises(ValueError):
        IVFBinaryIndex(ops.index_bin_max_dim() + 1, 4)
    with pytest.raises(ValueError):
        IVFBinaryIndex(0, 4)
    with pytest.raises(ValueError):
        IVFBinaryIndex(200, 0)
    for nprobe in (0, NL + 1):
        with pytest.raises(ValueError):
            ivf.search(q, 10, nprobe=nprobe)
    with pytest.raises(ValueError):
        ivf.search(q, 10, plan='gpu')
    fresh = IVFBinaryIndex(200, NL)
    with pytest.raises(ValueError):
        fresh.search(q, 10)                                      # before train
    with pytest.raises(ValueError):
        fresh.add(b)                                             # before train
    with pytest.raises(ValueError):
        fresh.save(str(tmp_path / 'no.npz'))                     # before train
    with pytest.raises(ValueError):
        fresh.train(b[:NL - 1])                                  # fewer rows than lists
    with pytest.raises(ValueError):
        ivf.train(b)                                             # rows already added
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, rerank=40)                   # no source
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, rerank=40, source=b[:, :199])    # a wrong source shape
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, rerank=9, source=b)          # R < k
    with pytest.raises(ValueError):
        ivf.search(q, 3001, nprobe=2)
    with pytest.raises(ValueError):
        ivf.search(q, 10, nprobe=2, same_set=True)
    with pytest.raises(ValueError):
        ivf.add(np.zeros((3, 199), np.float32))
    c, s = ops.quantize_rows(_cuda(q))
    probe = torch.zeros(33, 1, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.ivf_scan_bin(c, s, ivf.codes, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 257)       # bits too narrow
    with pytest.raises(ValueError):
        ops.ivf_scan_bin(c[:, :200], s, ivf.codes, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 200)   # codes below pad64(D)
    with pytest.raises(ValueError):
        ops.ivf_scan_bin(c, s, ivf.codes, ivf.scales, ivf.ids[:-1], ivf.list_off, probe, probe, 200)
    with pytest.raises(ValueError):
        ops.ivf_scan_bin(c, s, ivf.codes, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 200, qsums=ops.code_sums(c, 200)[:-1])
    with pytest.raises(TypeError):
        ops.ivf_scan_bin(c.to(torch.uint8), s, ivf.codes, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 200)
    with pytest.raises(TypeError):
        ops.ivf_scan_bin(c, s, ivf.codes.to(torch.int8), ivf.scales, ivf.ids, ivf.list_off, probe, probe, 200)
    with pytest.raises(TypeError):
        ops.ivf_scan_bin(c, s, ivf.codes, ivf.scales, ivf.ids, ivf.list_off, probe.long(), probe, 200)
    with pytest.raises(TypeError):
        ops.code_sums(c.to(torch.uint8), 200)
    with pytest.raises(ValueError):
        ops.code_sums(c, 257)


# ---- python -m dirtorch_amd.retrieve --index ivfbin, ranking.expand_device(index=IVFBinaryIndex) -----------------------
def test_retrieve_cli_with_a_binary_inverted_file(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): --index ivfbin --nlist 8 --nprobe 3 [--rerank 28]
    writes what the class gives for the same descriptors, and with every list probed what --index bin stands for."""
    import dir_oracle as O
    from dirtorch_amd.index import IVFBinaryIndex
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
    runs = {'rerank': ['--nprobe', '3', '--rerank', '28'], 'raw': ['--nprobe', '3'], 'all': ['--nprobe', '8']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', outs[name], '--index', 'ivfbin', '--nlist', '8'] + flags, env=env)
             for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0, 0]
    index = IVFBinaryIndex(D, 8).train(x).add(x)
    for name, kw in (('rerank', dict(nprobe=3, rerank=28, source=x)), ('raw', dict(nprobe=3)), ('all', dict(nprobe=8))):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in index.search(x, k, same_set=True, **kw)), name)
        assert (npz['idx'] != np.arange(N)[:, None]).all()
    npz = np.load(outs['all'])
    _same((npz['idx'], npz['scores']), bin_ref.search(x, x, k, exclude=np.arange(N)), 'every list probed: the flat binary lists')


def test_expand_device_takes_a_binary_inverted_file(sets):
    """ranking.expand_device(index=IVFBinaryIndex) needs no change: it equals the route with the lists made by hand."""
    from dirtorch_amd import ops, ranking
    from dirtorch_amd.index import IVFBinaryIndex
    b = sets['b'][:600]
    index = IVFBinaryIndex(200, 8).train(b).add(b)
    for kw in (dict(nprobe=2), dict(nprobe=2, rerank=32)):
        got = ranking.expand_device(b, alpha=2, k=8, index=index, **kw)
        idx, vals = index.search(b, 8, same_set=True, **(dict(kw, source=_cuda(b)) if 'rerank' in kw else kw))
        want = ops.expand_lists(_cuda(b), _cuda(b), idx, vals, 2.0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    q = sets['q']
    got = ranking.expand_device(q, db=b, alpha=1, k=5, index=index, nprobe=3)
    want = ops.expand_lists(_cuda(q), _cuda(b), *index.search(q, 5, nprobe=3), 1.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))

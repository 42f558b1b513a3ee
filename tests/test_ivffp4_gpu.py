"""The inverted file over fp4 codes on the device (dir_ivf_scan_fp4, index.IVFFp4Index, python -m dirtorch_amd.retrieve
--index ivffp4).  A score is dir_similarity_fp4's number - an exact sum times two fp32 factors - whatever the cut of the work,
so every comparison is on bits: the scan with tests/fp4_ref.py's scores, a search over every list with Fp4Index.search, a
search over fewer lists and the list-major store with the numpy restatement of tests/ivffp4_ref.py on the device-trained
centroids."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fp4_ref
import ivffp4_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8(a):
    return _cuda(a, np.uint8)


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- ivf_scan_fp4 ------------------------------------------------------------------------------------------------------
LENS = [0, 1, 255, 256, 257, 0, 700, 31, 300]      # a tile of the scan is 256 rows: one short of it, one, one and a row, three
NLIST, NROWS = len(LENS), sum(LENS)
LIST_OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
GAP, PAST, FILL = 2, 7, 12345                      # empty columns between slots, columns past the width, what they hold


def _coded(r, n, D, junk=False):
    """random stored rows (codes [n, ldc], exps [n, lde]): every nibble, -0 included, and the three block levels; junk: the
    codes past D hold noise, the block bytes past D anything but 255 and those past D rounded up to 64 are 255"""
    ldc, lde = fp4_ref.widths(D)
    nib = np.zeros((n, 2 * ldc), np.uint8)
    if junk:
        nib[:] = r.randint(0, 16, nib.shape)
    nib[:, :D] = r.randint(0, 16, (n, D))
    exps = np.full((n, lde), 127, np.uint8)
    if junk:
        exps[:] = r.randint(0, 255, exps.shape)
        exps[:, (D + 63) // 64 * 2:] = 255
    exps[:, :(D + 31) // 32] = r.randint(125, 128, (n, (D + 31) // 32))
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), exps


def _clean(codes, exps, D):
    """the stored rows as the definition reads them: nothing past D"""
    codes, exps = codes.copy(), exps.copy()
    codes[:, (D + 1) // 2:] = 0
    if D % 2:
        codes[:, D // 2] &= 0x0f
    exps[:, (D + 31) // 32:] = 127
    return codes, exps


def _check_scan(dev, D, want, ids, probe):
    """One ops.ivf_scan_fp4 call on the table `probe` [Q, nprobe] (slots GAP columns apart, in a buffer PAST columns wider
    than the stated width) against the flat scores `want` [Q, NROWS]: ids of every column, score bits of every covered one;
    then the call that sizes its rows itself (width=None) and the call on caller-made tables."""
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
    dq, deq, dsq, db, deb, dsb, dids, doff = dev
    dprobe, dcol = _cuda(probe, np.int32), _cuda(col_off, np.int32)
    got_s, got_i = ops.ivf_scan_fp4(dq[:Q], deq[:Q], dsq[:Q], db, deb, dsb, dids, doff, dprobe, dcol, D, width=width,
                                    out=(scores, out_ids))
    assert got_s.data_ptr() == scores.data_ptr() and tuple(got_s.shape) == (Q, width) == tuple(got_i.shape)
    gi, gs = out_ids.cpu().numpy(), scores.cpu().numpy()
    assert (gi[:, :width] == exp_ids).all(), np.argwhere(gi[:, :width] != exp_ids)[:5]
    ok = _bits_equal(gs[:, :width], exp_scores)
    assert ok[covered].all(), np.argwhere(~ok & covered)[:5]
    assert (gi[:, width:] == FILL).all() and (gs[:, width:] == FILL).all()
    # without `out` and `width`: the call sizes the rows itself
    got_s, got_i = ops.ivf_scan_fp4(dq[:Q], deq[:Q], dsq[:Q], db, deb, dsb, dids, doff, dprobe, dcol, D)
    assert tuple(got_i.shape) == (Q, width - 3) and (got_i.cpu().numpy() == exp_ids[:, :width - 3]).all()
    ok = _bits_equal(got_s.cpu().numpy(), exp_scores[:, :width - 3])
    assert ok[covered[:, :width - 3]].all()
    # ... and with the probe tables prepared by the caller
    tables = ops.ivf_probe_tables(doff, dprobe, dcol)
    assert tables[5] == width - 3 and all(t.dtype == torch.int32 and t.is_cuda for t in tables[:4])
    again_s, again_i = ops.ivf_scan_fp4(dq[:Q], deq[:Q], dsq[:Q], db, deb, dsb, dids, doff, dprobe, dcol, D, tables=tables)
    assert torch.equal(again_i, got_i) and torch.equal(again_s.view(torch.int32)[again_i >= 0], got_s.view(torch.int32)[got_i >= 0])


@pytest.mark.parametrize('D', [1, 33, 96, 160, 256, 257, 1024, 1280, 2048])
def test_ivf_scan_fp4_is_the_restatement(D):
    """Hand-made lists, no training: every covered column carries fp4_ref.score's bits and its row's id, every other
    column id -1, and nothing past the width is written.  Q = 1 / 33 / 97 / 200 queries with 1 / 3 / 9 distinct random
    lists each (-1 in some slots); 200 queries that all probe the 700-row list (seven groups of 32 per tile); a table
    that leaves lists out; no list at all; one NaN scale on each side; in the database's padding noise in the codes past
    D and in the block bytes past D, 0xFF in those of the blocks past D rounded up to 64.  D = 1: the smallest row, 33: a
    second block, 96 / 160: 4 / 6 of a slab's 8 chunks (both sides cut by chunk), 256: one full slab, 257: two slabs, the
    last with 2 chunks, 1024: four slabs (the ring full), 1280: five (the ring wraps), 2048: the full row."""
    r = np.random.RandomState(280 + D)
    cq, eq = _coded(r, 200, D)
    cb, eb = _coded(r, NROWS, D, junk=True)
    sq = np.exp(r.uniform(-8, 2, 200)).astype(np.float32)
    sb = np.exp(r.uniform(-8, 2, NROWS)).astype(np.float32)
    sb[5], sq[7] = np.nan, np.nan
    ids = r.permutation(NROWS).astype(np.int32)
    want = fp4_ref.score(cq, eq, sq, *_clean(cb, eb, D), sb, D)
    dev = (_u8(cq), _u8(eq), _cuda(sq), _u8(cb), _u8(eb), _cuda(sb), _cuda(ids, np.int32), _cuda(LIST_OFF, np.int32))
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


def test_accumulation_is_exact_at_the_bound():
    """D = 7281, the widest row (29 slabs): every code +-6 under the block byte 127, one sign per row, so every accumulator
    is +-36 * 7281 = +-262116 - a sum whose partial sums need all 24 bits - compared on bits.  Two lists, of 3 and of 40
    rows, five queries that probe both."""
    from dirtorch_amd import ops
    D = fp4_ref.MAX_DIM
    ldc, lde = fp4_ref.widths(D)
    r = np.random.RandomState(290)
    Q, N = 5, 43

    def rows(neg):
        nib = np.zeros((len(neg), 2 * ldc), np.uint8)
        nib[:, :D] = np.where(neg, 15, 7)[:, None]
        return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), np.full((len(neg), lde), 127, np.uint8)

    qneg, bneg = np.array([0, 1, 0, 1, 1], bool), r.randint(0, 2, N).astype(bool)
    (cq, eq), (cb, eb) = rows(qneg), rows(bneg)
    acc = fp4_ref.acc(cq, eq, cb, eb, D)
    assert (acc == np.where(qneg[:, None] ^ bneg[None, :], -1, 1) * np.float32(36 * D)).all() and 36 * D * 64 == 2 ** 24 - 1792
    one = np.ones(N, np.float32)
    list_off = np.array([0, 3, 43], np.int32)
    probe = np.tile(np.array([[1, 0]], np.int32), (Q, 1))
    col_off = np.tile(np.array([[0, 40]], np.int32), (Q, 1))
    ids = r.permutation(N).astype(np.int32)
    got_s, got_i = ops.ivf_scan_fp4(_u8(cq), _u8(eq), _cuda(one[:Q]), _u8(cb), _u8(eb), _cuda(one), _cuda(ids, np.int32),
                                    _cuda(list_off, np.int32), _cuda(probe, np.int32), _cuda(col_off, np.int32), D)
    order = np.concatenate([np.arange(3, 43), np.arange(3)])
    assert tuple(got_s.shape) == (Q, 43) and (got_i.cpu().numpy() == ids[order][None, :]).all()
    assert (bits(got_s.cpu().numpy()) == bits(acc[:, order])).all()


# ---- IVFFp4Index -------------------------------------------------------------------------------------------------------
NL = 16


@pytest.fixture(scope='module')
def sets():
    """fp4_ref.rerank_sets() - the inputs tests/test_ivffp4_cpu.py checks the fixture conditions on - a device-trained index
    over them, the flat fp4 index of the same rows and the trained centroids on the host."""
    from dirtorch_amd.index import Fp4Index, IVFFp4Index
    q, b = fp4_ref.rerank_sets()
    ivf = IVFFp4Index(200, NL).train(b, iters=10, seed=0).add(b)
    return dict(q=q, b=b, ivf=ivf, flat=Fp4Index(200).add(b), centroids=ivf.centroids.cpu().numpy())


def test_every_list_probed_gives_the_flat_fp4_index_lists(sets, tmp_path):
    from dirtorch_amd.index import IVFInt8Index
    q, b, ivf, flat = sets['q'], sets['b'], sets['ivf'], sets['flat']
    assert len(ivf) == 3000 and ivf.nlist == NL and ivf.nbytes() == 3000 * (128 + 8 + 4 + 4)
    i8 = IVFInt8Index(200, NL).train(b, iters=10, seed=0)                 # the coarse side is the int8 inverted file's
    assert torch.equal(i8.centroids.view(torch.int32), ivf.centroids.view(torch.int32)) and torch.equal(i8.ccodes, ivf.ccodes)
    for k in (10, 100):
        want = flat.search(q, k)
        _same(want, fp4_ref.search(q, b, k))
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
    from dirtorch_amd.index import Fp4Index, IVFFp4Index
    b = sets['b'][:600]
    ivf, flat = IVFFp4Index(200, 8).train(b).add(b), Fp4Index(200).add(b)
    for k, kw in ((20, {}), (20, dict(scratch_bytes=8 * 600 * 250)), (600, {})):
        idx, vals = ivf.search(b, k, nprobe=8, same_set=True, **kw)
        _same((idx, vals), flat.search(b, k, same_set=True), 'k = %d' % k)
        assert (idx.cpu().numpy() != np.arange(600)[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    _same(ivf.search(b, 20, nprobe=8, rerank=80, source=b, same_set=True), flat.search(b, 20, rerank=80, source=b, same_set=True))


def test_the_store_is_the_restatements_and_does_not_depend_on_the_add_calls(sets):
    """One call, three calls and three calls of mixed kinds (ndarray, CPU tensor, CUDA tensor) build the same list-major
    store, which is the restatement's on the device-trained centroids - ids ascending inside every list."""
    from dirtorch_amd.index import IVFFp4Index
    q, b, one = sets['q'], sets['b'], sets['ivf']
    want = ivffp4_ref.build(b, sets['centroids'])
    assert (one.ids.cpu().numpy() == want['ids']).all() and (one.list_off.cpu().numpy() == want['list_off']).all()
    assert (one.codes.cpu().numpy() == want['codes']).all() and (one.exps.cpu().numpy() == want['exps']).all()
    assert (bits(one.scales.cpu().numpy()) == bits(want['scales'])).all()
    lens = np.diff(want['list_off'])
    assert lens.max() > 256 and lens.min() < 64
    for parts in ((b[:1000], b[1000:1001], b[1001:]),
                  (b[:1000], torch.from_numpy(b[1000:1001]), torch.from_numpy(b[1001:]).cuda())):
        index = IVFFp4Index(200, NL)
        index._set_centroids(one.centroids.clone())
        for part in parts:
            index.add(part)
        assert len(index) == 3000
        for name in ('codes', 'exps', 'ids', 'list_off'):
            assert torch.equal(getattr(index, name), getattr(one, name)), name
        assert torch.equal(index.scales.view(torch.int32), one.scales.view(torch.int32))
        _same(index.search(q, 10, nprobe=NL), sets['flat'].search(q, 10))
        _same(index.search(q, 10, nprobe=2), one.search(q, 10, nprobe=2))


@pytest.mark.parametrize('nprobe', [1, 2, 4])
def test_probed_search_is_the_restatement(sets, nprobe):
    """Given the centroids the whole search is defined: the lists equal ivffp4_ref's masked search, ids and value bits,
    including the rows that run short at k = 100, nprobe = 1."""
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    for k in (10, 100):
        want = ivffp4_ref.search(q, b, sets['centroids'], k, nprobe)
        for kw in ({}, dict(scratch_bytes=8 * 400 * 5)):
            _same(ivf.search(q, k, nprobe=nprobe, **kw), want, 'k = %d, %r' % (k, kw))
    if nprobe == 1:
        assert (want[0][:, -1] == -1).any() and (want[0][:, 0] >= 0).all()
    own = np.arange(33, dtype=np.int32) * 7
    qq = b[own]                                                          # queries that ARE rows
    _same(ivf.search(qq, 10, nprobe=nprobe), ivffp4_ref.search(qq, b, sets['centroids'], 10, nprobe))


def test_search_pads_a_chunk_whose_rows_all_run_short():
    """Forty rows in four hand-set lists of 10, 4, 14 and 12 (no training), k = 40: with one list probed a query has 4 - 14
    neighbours, with two 14 - 26, so every chunk of queries is narrower than k and search widens it with empty columns
    before the top-k.  The lists equal ivffp4_ref's, ids and value bits with their (-1, NaN) tails, in one chunk and in
    chunks of two queries."""
    from dirtorch_amd.index import IVFFp4Index
    b, q = synth_descriptors(6, 3000, 200)[:40], synth_descriptors(5, 33, 200)[:5]
    c = b[[0, 10, 20, 30]]
    index = IVFFp4Index(200, 4)
    index._set_centroids(_cuda(c))
    index.add(b)
    assert index._lens.tolist() == [10, 4, 14, 12] == np.diff(ivffp4_ref.build(b, c)['list_off']).tolist()
    for nprobe, least, most in ((1, 4, 14), (2, 14, 26)):
        want = ivffp4_ref.search(q, b, c, 40, nprobe)
        found = (want[0] >= 0).sum(axis=1)
        assert found.min() == least and found.max() == most and most < 40         # every query runs short
        assert (want[0][:, most:] == -1).all() and np.isnan(want[1][:, most:]).all()
        for kw in ({}, dict(scratch_bytes=2 * (8 * 40 + 128 + 8 + 4))):             # two queries: 40 columns and their fp4 codes
            _same(index.search(q, 40, nprobe=nprobe, **kw), want, 'nprobe = %d, %r' % (nprobe, kw))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd import ops
    from dirtorch_amd.index import Fp4Index, IVFFp4Index
    q, b, ivf = sets['q'], sets['b'], sets['ivf']
    path = str(tmp_path / 'ivffp4.npz')
    ivf.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'centroids', 'codes', 'exps', 'ids', 'list_off', 'nlist', 'scales']
        assert f['codes'].shape == (3000, 100) and f['codes'].dtype == np.uint8 and f['exps'].shape == (3000, 7)
        assert f['centroids'].shape == (NL, 200) and f['ids'].dtype == np.int32 and f['list_off'].shape == (NL + 1,)
    back = IVFFp4Index.load(path)
    assert back.D == 200 and back.nlist == NL and len(back) == 3000 and back.nbytes() == ivf.nbytes()
    for name in ('codes', 'exps', 'ids', 'list_off', 'ccodes'):
        assert torch.equal(getattr(back, name), getattr(ivf, name)), name
    for name in ('scales', 'centroids', 'cscales'):
        assert torch.equal(getattr(back, name).view(torch.int32), getattr(ivf, name).view(torch.int32)), name
    for kw in (dict(nprobe=2), dict(nprobe=NL, rerank=40, source=_cuda(b))):
        _same(back.search(q, 10, **kw), ivf.search(q, 10, **kw))
    # the fp4 half of the file is Fp4Index's format: the flat index reads the list-major rows as they lie
    flat = Fp4Index.load(path)
    assert torch.equal(flat.codes, ivf.codes) and torch.equal(flat.exps, ivf.exps)
    with pytest.raises(ValueError):
        IVFFp4Index(ops.index_fp4_max_dim() + 1, 4)              # D = 7282
    with pytest.raises(ValueError):
        IVFFp4Index(0, 4)
    with pytest.raises(ValueError):
        IVFFp4Index(200, 0)
    for nprobe in (0, NL + 1):
        with pytest.raises(ValueError):
            ivf.search(q, 10, nprobe=nprobe)
    fresh = IVFFp4Index(200, NL)
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
    c, e, s = ops.quantize_rows_fp4(_cuda(q))
    probe = torch.zeros(33, 1, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError):
        ops.ivf_scan_fp4(c, e, s, ivf.codes, ivf.exps, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 257)   # codes too narrow
    with pytest.raises(ValueError):
        ops.ivf_scan_fp4(c, e, s, ivf.codes, ivf.exps, ivf.scales, ivf.ids[:-1], ivf.list_off, probe, probe, 200)
    with pytest.raises(TypeError):
        ops.ivf_scan_fp4(c.to(torch.int8), e, s, ivf.codes, ivf.exps, ivf.scales, ivf.ids, ivf.list_off, probe, probe, 200)
    with pytest.raises(TypeError):
        ops.ivf_scan_fp4(c, e, s, ivf.codes, ivf.exps, ivf.scales, ivf.ids, ivf.list_off, probe.long(), probe, 200)


# ---- python -m dirtorch_amd.retrieve --index ivffp4, ranking.expand_device(index=IVFFp4Index) --------------------------
def test_retrieve_cli_with_an_fp4_inverted_file(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): --index ivffp4 --nlist 8 --nprobe 3 [--rerank 28]
    writes what the class gives for the same descriptors, and with every list probed what --index fp4 stands for."""
    import dir_oracle as O
    from dirtorch_amd.index import IVFFp4Index
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
                               '--topk', str(k), '--output', outs[name], '--index', 'ivffp4', '--nlist', '8'] + flags, env=env)
             for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0, 0]
    index = IVFFp4Index(D, 8).train(x).add(x)
    for name, kw in (('rerank', dict(nprobe=3, rerank=28, source=x)), ('raw', dict(nprobe=3)), ('all', dict(nprobe=8))):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in index.search(x, k, same_set=True, **kw)), name)
        assert (npz['idx'] != np.arange(N)[:, None]).all()
    npz = np.load(outs['all'])
    _same((npz['idx'], npz['scores']), fp4_ref.search(x, x, k, exclude=np.arange(N)), 'every list probed: the flat fp4 lists')


def test_expand_device_takes_an_fp4_inverted_file(sets):
    """ranking.expand_device(index=IVFFp4Index) needs no change: it equals the route with the lists made by hand."""
    from dirtorch_amd import ops, ranking
    from dirtorch_amd.index import IVFFp4Index
    b = sets['b'][:600]
    index = IVFFp4Index(200, 8).train(b).add(b)
    for kw in (dict(nprobe=2), dict(nprobe=2, rerank=32)):
        got = ranking.expand_device(b, alpha=2, k=8, index=index, **kw)
        idx, vals = index.search(b, 8, same_set=True, **(dict(kw, source=_cuda(b)) if 'rerank' in kw else kw))
        want = ops.expand_lists(_cuda(b), _cuda(b), idx, vals, 2.0)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    q = sets['q']
    got = ranking.expand_device(q, db=b, alpha=1, k=5, index=index, nprobe=3)
    want = ops.expand_lists(_cuda(q), _cuda(b), *index.search(q, 5, nprobe=3), 1.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))

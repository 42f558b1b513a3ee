"""The binary descriptor index on the device (dir_quantize_rows_bin, dir_similarity_bin, index.BinaryIndex, python -m
dirtorch_amd.retrieve --index bin) against the numpy restatement of tests/bin_ref.py.  The scale is a fixed chain of
single fp32 operations and the sum of a score an exact int32 below 2^24, so bits, scales, scores and the lists of a scan
are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bin_ref
import index_ref
from index_util import cuda as _cuda, same as _same
from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QB, ROWS = 96, 256      # csrc/index_bin.hip: query rows per block, database rows per workgroup


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def _u8(a):
    return _cuda(a, np.uint8)


def _i8(a):
    return _cuda(a, np.int8)


# ---- quantize_rows_bin -------------------------------------------------------------------------------------------------
def _check_quantize(x, pitch=0, offset=0, what=''):
    """ops.quantize_rows_bin against the restatement; the output buffers are likely to reuse a block full of 0x55, so a
    padding byte the kernel does not write shows.  pitch: the rows lie at D + pitch floats; offset: ... from float `offset`
    of an allocation (1: the rows are not 16-byte aligned)."""
    from dirtorch_amd import ops
    N, D = x.shape
    dev = _cuda(x)
    if pitch or offset:
        wide = torch.full((N * (D + pitch) + offset,), float('nan'), dtype=torch.float32, device='cuda')
        view = wide[offset:].view(N, D + pitch)[:, :D]
        view.copy_(dev)
        dev = view
    junk = torch.full((N, bin_ref.width(D)), 0x55, dtype=torch.uint8, device='cuda')
    del junk
    got_bits, got_scales = ops.quantize_rows_bin(dev)
    assert got_bits.dtype == torch.uint8 and got_scales.dtype == torch.float32
    assert tuple(got_bits.shape) == (N, bin_ref.width(D)) and tuple(got_scales.shape) == (N,)
    got_bits, got_scales = got_bits.cpu().numpy(), got_scales.cpu().numpy()
    want_bits, want_scales = bin_ref.quantize(x)
    assert (got_bits == want_bits).all(), (what, np.argwhere(got_bits != want_bits)[:5])
    assert _bits_equal(got_scales, want_scales).all(), (what, np.argwhere(~_bits_equal(got_scales, want_scales))[:5])
    return got_bits, got_scales


@pytest.mark.parametrize('D', [1, 7, 64, 127, 128, 129, 200, 1000, 2048, 2049, 4100])
def test_quantize_rows_matches_the_restatement(D):
    """One wave per row, four rows per workgroup, eight lanes per dword of bits; 2048 values is what a wave keeps in
    registers (2049, 4100: the two-pass form); pitched and unaligned inputs take the scalar loads.  Rows 0 .. 3 of the
    second set: -0.0 among the values, a zero row, a row with an infinity, a row with a NaN."""
    r = np.random.RandomState(280 + D)
    for N in (5, 261):
        x = (r.standard_normal((N, D)) * np.exp(r.uniform(-12, 12, (N, 1)))).astype(np.float32)
        _check_quantize(x, what='%d x %d' % (N, D))
    x = (r.standard_normal((41, D)) * np.exp(r.uniform(-3, 3, (41, 1)))).astype(np.float32)
    x[0, ::2] = -0.0
    x[1] = 0
    x[2, D - 1] = -np.inf
    x[3, D // 2] = np.nan
    x[4] = -0.0
    for pitch, offset in ((0, 0), (3, 0), (4, 0), (0, 1), (4, 2)):
        got_bits, got_scales = _check_quantize(x, pitch=pitch, offset=offset, what='pitch D + %d, offset %d' % (pitch, offset))
    assert not got_bits[1:5].any() and (bits(got_scales[[1, 4]]) == 0).all() and np.isnan(got_scales[2:4]).all()
    if D > 1:
        assert not (got_bits[0] & 0x55).any()                                            # the even k are -0.0: bit clear


# ---- similarity_bin ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [128, 1024, 1152, 2048])
def test_scan_layout_one_hot_pairs(D):
    """Query i is one-hot at k = i; database row j holds the single bit k' = (a j + s) mod D, once with (a, s) = (1, 0)
    and once with (7, 3), so k and k' walk every position of a slab, the slab edge (D = 1152: a whole slab and one
    chunk; 2048: two slabs) and every row of a tile with every k.  t = +code where k == k', -code elsewhere: a wrong
    bit-to-byte order, chunk, lane half or slab moves the positive cell."""
    from dirtorch_amd import ops
    i = np.arange(D)
    code = (1 + i % 127) * np.where(i % 3 == 1, -1, 1)
    qc = np.zeros((D, D), np.int8)
    qc[i, i] = code
    one = torch.ones(D, dtype=torch.float32, device='cuda')
    dq = _i8(qc)
    for a, s in ((1, 0), (7, 3)):
        kb = (a * i + s) % D
        rows = np.zeros((D, bin_ref.width(D)), np.uint8)
        rows[i, kb >> 3] = 1 << (kb & 7)
        got = ops.similarity_bin(dq, one, _u8(rows), one, D).cpu().numpy()
        hit = i[:, None] == kb[None, :]
        want = np.where(hit, code[:, None], -code[:, None]).astype(np.float32)
        assert (got == want).all(), (a, s, np.argwhere(got != want)[:5])
        assert (bits(got) == bits(bin_ref.score(qc, np.ones(D), rows, np.ones(D), D))).all()


@pytest.mark.parametrize('D', [64, 200, 1000, 1024, 1088, 2048, 2176])
def test_similarity_bin_is_the_restatement(D):
    """grid = (database tiles of 256 rows, query blocks of 96 rows), sub-slabs of 128 k, database slabs of 1024.  D = 64,
    200, 1000: one slab cut to 1, 2, 8 chunks with a partial last sub-slab; 1024: one whole slab; 1088: a slab and a
    chunk; 2048: two slabs, the resident form; 2176: three slabs, where the database ring turns.  The query codes are
    noise past D (ldq > D) and the database bits are noise past D: neither may count.  A NaN and a zero scale."""
    from dirtorch_amd import ops
    r = np.random.RandomState(300 + D)
    ldq, ldb = D + 70, bin_ref.width(D)
    qc = r.randint(-127, 128, (97, ldq)).astype(np.int8)
    qc[0, :D], qc[1, :D] = 127, -127
    rows = r.randint(0, 256, (513, ldb)).astype(np.uint8)
    rows[0], rows[1] = 0xff, 0
    sq = np.exp2(r.randint(-20, 5, 97)).astype(np.float32)
    sb = (np.exp2(r.randint(-20, 5, 513)) * r.uniform(1, 2, 513)).astype(np.float32)
    sb[5], sb[7], sq[3] = np.nan, 0, 0
    want = bin_ref.score(qc, sq, rows, sb, D)
    dq, ds, db, dbs = _i8(qc), _cuda(sq), _u8(rows), _cuda(sb)
    for Q in (1, QB, QB + 1):
        for N in (1, ROWS - 1, ROWS, ROWS + 1, 513):
            got = ops.similarity_bin(dq[:Q], ds[:Q], db[:N], dbs[:N], D)
            assert got.dtype == torch.float32 and tuple(got.shape) == (Q, N)
            g = got.cpu().numpy()
            assert _bits_equal(g, want[:Q, :N]).all(), (Q, N, np.argwhere(~_bits_equal(g, want[:Q, :N]))[:5])
    # a score pitch lds > N: the columns past N stay as they were; database rows from a row offset
    out = torch.full((97, 300), -7.0, dtype=torch.float32, device='cuda')
    got = ops.similarity_bin(dq, ds, db[3:260], dbs[3:260], D, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (97, 257)
    assert _bits_equal(got.cpu().numpy(), want[:, 3:260]).all() and (out[:, 257:] == -7).all()
    # rows at a pitch wider than their width, noise in between
    wide = torch.full((513, ldb + 48), 0xff, dtype=torch.uint8, device='cuda')
    wide[:, :ldb] = db
    got = ops.similarity_bin(dq, ds, wide[:, :ldb], dbs, D)
    assert _bits_equal(got.cpu().numpy(), want).all()


def test_the_sum_is_exact_up_to_the_bound():
    """D = 131072, the widest row (128 database slabs).  Every query code +-127 against rows of all ones, all zeros and
    alternating bits: |t| = 127 * D = 16 646 144 needs all 24 bits of the fp32 it becomes, and the kernel's
    2 * sum - qsum passes through twice that in int32."""
    from dirtorch_amd import ops
    D = bin_ref.MAX_DIM
    r = np.random.RandomState(310)
    Q, N = 2, 300
    qc = np.full((Q, D), 127, np.int8)
    qc[1, 1::2] = -127
    rows = r.randint(0, 256, (N, bin_ref.width(D))).astype(np.uint8)
    rows[0], rows[1], rows[2], rows[3] = 0xff, 0, 0x55, 0xaa
    rows[299] = 0xff
    t = bin_ref.dot(qc, rows, D)
    assert t[0, 0] == 127 * D == 16646144 and t[0, 1] == -127 * D and t[0, 2] == 0 and t[1, 2] == 127 * D and t[1, 3] == -127 * D
    one = np.ones(N, np.float32)
    got = ops.similarity_bin(_i8(qc), _cuda(one[:Q]), _u8(rows), _cuda(one), D).cpu().numpy()
    assert (got.astype(np.int64) == t).all(), np.argwhere(got.astype(np.int64) != t)[:5]
    sq, sb = np.exp2(r.randint(-30, 30, Q)).astype(np.float32), r.uniform(0.5, 2, N).astype(np.float32)
    got = ops.similarity_bin(_i8(qc), _cuda(sq), _u8(rows), _cuda(sb), D).cpu().numpy()
    assert (bits(got) == bits(bin_ref.score(qc, sq, rows, sb, D))).all()


# ---- BinaryIndex -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sets():
    """The inputs tests/test_bin_cpu.py checks the re-rank condition on, their quantised and exact scores."""
    q, b = bin_ref.rerank_sets()
    quant = bin_ref.score(*index_ref.quantize(q), *bin_ref.quantize(b), 200)
    exact64 = q.astype(np.float64) @ b.astype(np.float64).T
    mass = np.abs(q.astype(np.float64)) @ np.abs(b.astype(np.float64)).T            # sum_k |q_k b_k|
    return dict(q=q, b=b, quant=quant, exact64=exact64, exact=exact64.astype(np.float32), mass=mass)


def _index(b):
    from dirtorch_amd.index import BinaryIndex
    return BinaryIndex(b.shape[1]).add(b)


def test_search_is_the_restatement_however_the_work_is_cut(sets):
    """The lists are bin_ref.search's, value bits included, whether the database is scanned whole, in db_rows chunks or
    with a small scratch, and whether it was added in one call or in three calls of three input kinds."""
    from dirtorch_amd.index import BinaryIndex
    q, b = sets['q'], sets['b']
    one = _index(b)
    three = BinaryIndex(200)
    three.add(b[:1000])                                           # an ndarray,
    three.add(torch.from_numpy(b[1000:1001]))                     # a CPU tensor,
    three.add(torch.from_numpy(b[1001:]).cuda())                  # a CUDA tensor
    assert len(one) == len(three) == 3000
    assert torch.equal(one.codes, three.codes) and torch.equal(one.scales, three.scales)
    wb, ws = bin_ref.quantize(b)
    assert (one.codes.cpu().numpy() == wb).all() and (bits(one.scales.cpu().numpy()) == bits(ws)).all()
    assert one.nbytes() == 3000 * (32 + 4)
    for k in (10, 100):
        want = bin_ref.search(q, b, k)
        _same(want, topk_ref_rows(sets['quant'], k))
        for index in (one, three):
            for kw in ({}, dict(scratch_bytes=4 * 3000 * 10), dict(db_rows=701), dict(db_rows=701, scratch_bytes=4 * 701 * 10)):
                idx, vals = index.search(q, k, **kw)
                assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
                _same((idx, vals), want, '%r, k = %d' % (kw, k))


def test_search_same_set_and_short_rows(sets):
    b = sets['b'][:600]
    index = _index(b)
    own = np.arange(600, dtype=np.int32)
    for k, kw in ((20, {}), (20, dict(db_rows=177, scratch_bytes=4 * 177 * 250)), (600, {})):
        idx, vals = index.search(b, k, same_set=True, **kw)
        _same((idx, vals), bin_ref.search(b, b, k, exclude=own), 'k = %d' % k)
        assert (idx.cpu().numpy() != own[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    idx, vals = index.search(b, 600, rerank=600, source=_cuda(b), same_set=True)
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all() and (idx[:, :-1] >= 0).all()


def test_search_rerank_gives_retrieve_devices_lists(sets):
    """(k, R) = (10, 1280) and (100, 2048).  The precondition - the restatement's shortlist of R holds the exact top k of
    every query (tests/test_bin_cpu.py) - is asserted first; then the index's lists are retrieve_device's, and the values
    are within gather_scores' bound of the fp64 scores, from a device source and from a host one."""
    from dirtorch_amd import ranking
    q, b = sets['q'], sets['b']
    index = _index(b)
    rows = np.arange(33)[:, None]
    for k, R in ((10, 1280), (100, 2048)):
        want = topk_ref_rows(sets['exact'], k)[0]
        short = topk_ref_rows(sets['quant'], R)[0]
        assert all(set(want[i]) <= set(short[i]) for i in range(33))
        idx, vals = index.search(q, k, rerank=R, source=_cuda(b))
        got = idx.cpu().numpy()
        assert (got == want).all()
        assert (got == ranking.retrieve_device(q, b, k)[0].cpu().numpy()).all()
        err = np.abs(vals.cpu().numpy().astype(np.float64) - sets['exact64'][rows, got])
        assert (err <= 202 * 2.0 ** -24 * sets['mass'][rows, got]).all()
        idx2, vals2 = index.search(q, k, rerank=R, source=b, db_rows=2100)
        assert torch.equal(idx2, idx) and torch.equal(vals2.view(torch.int32), vals.view(torch.int32))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd import ops
    from dirtorch_amd.index import BinaryIndex
    q, b = sets['q'], sets['b']
    index = _index(b)
    path = str(tmp_path / 'index.npz')
    index.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'bits', 'scales']
        assert f['bits'].shape == (3000, 25) and f['bits'].dtype == np.uint8 and f['scales'].shape == (3000,)
    back = BinaryIndex.load(path)
    assert back.D == 200 and len(back) == 3000 and back.nbytes() == index.nbytes()
    assert torch.equal(back.codes, index.codes)
    assert torch.equal(back.scales.view(torch.int32), index.scales.view(torch.int32))
    for kw in (dict(), dict(rerank=40, source=_cuda(b))):
        a, c = index.search(q, 10, **kw), back.search(q, 10, **kw)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
    with pytest.raises(ValueError):
        BinaryIndex(ops.index_bin_max_dim() + 1)
    with pytest.raises(ValueError):
        BinaryIndex(0)
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=40)                           # no source
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=9, source=b)                  # R < k
    with pytest.raises(ValueError):
        index.search(q, 3001)
    with pytest.raises(ValueError):
        index.search(q, 10, same_set=True)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 199), np.float32))
    with pytest.raises(ValueError):
        ops.quantize_rows_bin(torch.zeros(2, ops.index_bin_max_dim() + 1, device='cuda'))
    c, s = ops.quantize_rows(_cuda(q))
    with pytest.raises(ValueError):
        ops.similarity_bin(c, s, index.codes, index.scales, 257)         # bits too narrow for that D
    with pytest.raises(TypeError):
        ops.similarity_bin(c.to(torch.uint8), s, index.codes, index.scales, 200)
    with pytest.raises(TypeError):
        ops.similarity_bin(c, s, index.codes.to(torch.int8), index.scales, 200)


# ---- python -m dirtorch_amd.retrieve --index bin, ranking.expand_device(index=BinaryIndex) -----------------------------
def test_retrieve_cli_with_a_binary_index(tmp_path):
    """The CLI in fresh processes on the synthetic descriptors of test_retrieve_cli_with_an_int8_index (--load-feats):
    with --index bin [--rerank 28] the .npz holds what BinaryIndex.search gives for the same descriptors."""
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
    runs = {'rerank': ['--index', 'bin', '--rerank', '28'], 'raw': ['--index', 'bin']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', outs[name]] + flags, env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    index = _index(x)
    for name, kw in (('rerank', dict(rerank=28, source=x)), ('raw', {})):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in index.search(x, k, same_set=True, **kw)), name)
        assert (npz['idx'] != np.arange(N)[:, None]).all()
    npz = np.load(outs['raw'])
    _same((npz['idx'], npz['scores']), bin_ref.search(x, x, k, exclude=np.arange(N)), 'raw lists')


def test_expand_device_takes_a_binary_index(sets):
    """ranking.expand_device(index=BinaryIndex) needs no change: it equals the list route fed the restatement's lists."""
    from dirtorch_amd import ops, ranking
    b = sets['b'][:600]
    index = _index(b)
    got = ranking.expand_device(b, alpha=2, k=8, index=index)
    idx, vals = bin_ref.search(b, b, 8, exclude=np.arange(600, dtype=np.int32))
    want = ops.expand_lists(_cuda(b), _cuda(b), _cuda(idx, np.int32), _cuda(vals), 2.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    got = ranking.expand_device(b, alpha=2, k=8, index=index, rerank=64)
    want = ops.expand_lists(_cuda(b), _cuda(b), *index.search(b, 8, rerank=64, source=_cuda(b), same_set=True), 2.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    q = sets['q']
    got = ranking.expand_device(q, db=b, alpha=1, k=5, index=index)
    idx, vals = bin_ref.search(q, b, 5)
    want = ops.expand_lists(_cuda(q), _cuda(b), _cuda(idx, np.int32), _cuda(vals), 1.0)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))

"""The int8 descriptor index on the device (dir_quantize_rows_i8, dir_similarity_i8, dir_gather_scores, index.Int8Index,
python -m dirtorch_amd.retrieve --index int8) against the numpy restatement of tests/index_ref.py.  An int8 dot product
accumulated in int32 is exact, so codes, scales, quantised scores and the lists of a scan are compared bit for bit; only
the fp32 re-score has a bound, the one include/dir_engine.h states."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import index_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QB, ROWS = 96, 256      # csrc/index_i8.hip: query rows per block, database rows per workgroup


def _bits_equal(got, want):
    """the same stored bits, a NaN matching any NaN (which NaN a multiply returns is not part of the definition)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ---- quantize_rows -----------------------------------------------------------------------------------------------------
def _quantize(x, pitch=0):
    """(codes, scales) ndarrays of ops.quantize_rows; the output buffers are likely to reuse a block full of 0x55, so a
    padding byte the kernel does not write shows."""
    from dirtorch_amd import ops
    N, D = x.shape
    dev = _cuda(x)
    if pitch:
        wide = torch.full((N, D + pitch), float('nan'), dtype=torch.float32, device='cuda')
        wide[:, :D] = dev
        dev = wide[:, :D]
    junk = torch.full((N, index_ref.pad64(D)), 0x55, dtype=torch.int8, device='cuda')
    del junk
    codes, scales = ops.quantize_rows(dev)
    assert codes.dtype == torch.int8 and scales.dtype == torch.float32 and codes.is_cuda and scales.is_cuda
    assert tuple(codes.shape) == (N, index_ref.pad64(D)) and tuple(scales.shape) == (N,)
    return codes.cpu().numpy(), scales.cpu().numpy()


def _check_quantize(x, pitch=0, what=''):
    codes, scales = _quantize(x, pitch)
    wc, ws = index_ref.quantize(x)
    assert (codes == wc).all(), (what, np.argwhere(codes != wc)[:5])
    assert (bits(scales) == bits(ws)).all(), (what, np.argwhere(bits(scales) != bits(ws))[:5])


@pytest.mark.parametrize('D', [1, 63, 64, 65, 200, 2048, 2500])
def test_quantize_rows_matches_the_restatement(D):
    """One wave per row, four rows per workgroup; 2048 values is what a wave keeps in registers (2500: the two-pass form)."""
    r = np.random.RandomState(80 + D)
    for N in (1, 257, 1000):
        x = (r.standard_normal((N, D)) * np.exp(r.uniform(-12, 12, (N, 1)))).astype(np.float32)
        _check_quantize(x, what='%d x %d' % (N, D))
    _check_quantize(synth_descriptors(6, 257, D), what='unit rows, D = %d' % D)


@pytest.mark.parametrize('D', [65, 200, 2048, 4100])
def test_quantize_rows_pitched_and_degenerate_rows(D):
    r = np.random.RandomState(90)
    x = r.standard_normal((41, D)).astype(np.float32)
    _check_quantize(x, pitch=3, what='pitch D + 3')               # (rows not 16-byte aligned: the scalar loads)
    _check_quantize(x, pitch=4, what='pitch D + 4')
    x[0] = 0
    x[1] = np.float32(1e-40) * r.randint(-3, 4, D)                # subnormals: 127 / amax overflows
    x[2] = np.float32(1e-36) * r.standard_normal(D)               # tiny but normal: products in the subnormal range
    x[3, D // 2] = np.nan
    x[4, D - 1] = np.inf
    x[5, 0] = -np.inf
    x[6] = -0.0
    x[7] = r.randint(-254, 255, D) * np.float32(0.5)              # amax = 127 -> inv = 1: entries at exactly half a step
    x[7, r.randint(D)] = 127
    x[8] = x[7] * np.float32(2.0 ** -20)
    codes, scales = _quantize(x)
    wc, ws = index_ref.quantize(x)
    assert (codes == wc).all() and (bits(scales) == bits(ws)).all()
    assert not codes[[0, 1, 3, 4, 5, 6]].any() and scales[0] == 0 and scales[1] == 0 and np.isnan(scales[3:6]).all()
    assert codes.min() >= -127
    half = np.flatnonzero(np.abs(x[7] * 2) % 2 == 1)
    assert len(half) > D // 4 and (codes[7, half] % 2 == 0).all()      # round half to even


# ---- similarity_i8 -----------------------------------------------------------------------------------------------------
def _codes(r, n, D, junk=False):
    """asymmetric random codes [n, ldc] over the whole range -127 .. 127; junk: the padding bytes hold noise"""
    c = np.zeros((n, index_ref.pad64(D)), np.int8)
    if junk:
        c[:] = r.randint(-127, 128, c.shape)
    c[:, :D] = r.randint(-127, 128, (n, D))
    return c


@pytest.mark.parametrize('D', [1, 64, 65, 129, 200, 320, 448, 640, 2048])
def test_similarity_i8_is_the_restatement(D):
    """One launch form: grid = (database tiles of 256 rows, query blocks of 96 rows), K slabs of 128 over D rounded up to
    64.  Q = 1 / 33 / 96 | 97 / 200: a partial block, a full one, one block plus a row, three blocks; N on both sides of a
    tile and twelve tiles (every rotation of the slab walk); D = 64, 129, 320: the last slab is half a slab, D = 65, 200:
    ragged, 448: four slabs, the last a half (the three-stage ring reuses its first slot), 640: five, 2048: sixteen slabs.  The database codes carry noise in their padding (it must not count)."""
    from dirtorch_amd import ops
    r = np.random.RandomState(100 + D)
    cq, cb = _codes(r, 200, D), _codes(r, 3000, D, junk=True)
    sq = np.exp(r.uniform(-8, 2, 200)).astype(np.float32)
    sb = np.exp(r.uniform(-8, 2, 3000)).astype(np.float32)
    sb[5] = np.nan
    want = index_ref.score(cq[:, :D], sq, cb[:, :D], sb)
    dq, dsq, db, dsb = _cuda(cq, np.int8), _cuda(sq), _cuda(cb, np.int8), _cuda(sb)
    for Q in (1, 33, QB, QB + 1, 200):
        for N in (1, ROWS - 1, ROWS, ROWS + 1, 3000):
            got = ops.similarity_i8(dq[:Q], dsq[:Q], db[:N], dsb[:N], D)
            assert got.dtype == torch.float32 and tuple(got.shape) == (Q, N)
            g = got.cpu().numpy()
            assert _bits_equal(g, want[:Q, :N]).all(), (Q, N, np.argwhere(~_bits_equal(g, want[:Q, :N]))[:5])
    # a score pitch lds > N: the columns past N stay as they were
    out = torch.full((97, 300), -7.0, dtype=torch.float32, device='cuda')
    got = ops.similarity_i8(dq[:97], dsq[:97], db[3:260], dsb[3:260], D, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (97, 257)
    assert _bits_equal(got.cpu().numpy(), want[:97, 3:260]).all() and (out[:, 257:] == -7).all()


def test_similarity_i8_accumulates_in_int32():
    """Dots beyond 2^24 (the float conversion rounds) and the largest int32 sum the index admits: both fail for a kernel
    that accumulates in fp32 or in a narrower integer."""
    from dirtorch_amd import ops
    r = np.random.RandomState(110)
    for D, Q, N in ((2112, 40, 300), (ops.index_i8_max_dim(), 3, 257)):
        cq = np.full((Q, D), 127, np.int8)
        cb = np.full((N, D), 127, np.int8)
        for n in range(1, N):                                     # row n: n * D / (4 N) entries flipped (row 0: none)
            cb[n, r.choice(D, n * D // (4 * N), replace=False)] = -127
        cq[1::2, ::3] = -127
        sq = np.exp(r.uniform(-1, 1, Q)).astype(np.float32)
        sb = np.exp(r.uniform(-1, 1, N)).astype(np.float32)
        dots = index_ref.dots(cq, cb)
        assert dots[0, 0] == 127 * 127 * D and (np.abs(dots) > 2 ** 24).sum() > Q * N // 4
        assert (dots.astype(np.float32).astype(np.int64) != dots).any()          # the conversion does round
        want = index_ref.score(cq, sq, cb, sb)
        got = ops.similarity_i8(_cuda(cq, np.int8), _cuda(sq), _cuda(cb, np.int8), _cuda(sb), D).cpu().numpy()
        assert (bits(got) == bits(want)).all(), (D, np.argwhere(bits(got) != bits(want))[:5])
    assert dots[0, 0] == 2114060288


# ---- gather_scores -----------------------------------------------------------------------------------------------------
def _cand(r, Q, R, N):
    cand = r.randint(0, N, (Q, R)).astype(np.int32)
    cand[r.rand(Q, R) < 0.1] = -1
    return cand


def _gather_ref(q, b, cand):
    """fp64 scores and sum_k |q_k b_k| of the candidates; -1 -> NaN"""
    s, a = np.empty(cand.shape), np.empty(cand.shape)
    for i in range(len(q)):
        prod = b[np.maximum(cand[i], 0)].astype(np.float64) * q[i].astype(np.float64)
        s[i], a[i] = prod.sum(axis=1), np.abs(prod).sum(axis=1)
    s[cand < 0] = np.nan
    return s, a


@pytest.mark.parametrize('D', [1, 63, 200, 2048])
def test_gather_scores_exact_on_small_integers(D):
    """Operands in [-3, 3]: every product and every partial sum is an integer below 2^24, exact in fp32 in any order."""
    from dirtorch_amd import _lib, ops
    r = np.random.RandomState(120 + D)
    Q, N, R = 7, 300, 37
    q, b = r.randint(-3, 4, (Q, D)).astype(np.float32), r.randint(-3, 4, (N, D)).astype(np.float32)
    cand = _cand(r, Q, R, N)
    want = _gather_ref(q, b, cand)[0].astype(np.float32)
    got = ops.gather_scores(_cuda(q), _cuda(b), _cuda(cand, np.int32))
    assert got.dtype == torch.float32 and tuple(got.shape) == (Q, R)
    g = got.cpu().numpy()
    assert (np.isnan(g) == (cand < 0)).all() and (g[cand >= 0] == want[cand >= 0]).all()
    # pitched everything: queries, database and cand through the wrapper, the scores through the C ABI
    wq = torch.full((Q, D + 3), float('nan'), device='cuda')
    wb = torch.full((N, D + 5), float('nan'), device='cuda')
    wc = torch.full((Q, R + 4), 2 ** 30, dtype=torch.int32, device='cuda')
    wq[:, :D], wb[:, :D], wc[:, :R] = _cuda(q), _cuda(b), _cuda(cand, np.int32)
    g = ops.gather_scores(wq[:, :D], wb[:, :D], wc[:, :R]).cpu().numpy()
    assert (np.isnan(g) == (cand < 0)).all() and (g[cand >= 0] == want[cand >= 0]).all()
    ws = torch.full((Q, R + 6), -7.0, device='cuda')
    _lib.call('dir_gather_scores', _lib.ptr(wq), D + 3, Q, _lib.ptr(wb), D + 5, N, D, _lib.ptr(wc), R + 4, R, _lib.ptr(ws),
              R + 6, _lib.stream_ptr())
    g = ws.cpu().numpy()
    assert (np.isnan(g[:, :R]) == (cand < 0)).all() and (g[:, :R][cand >= 0] == want[cand >= 0]).all()
    assert (g[:, R:] == -7).all()


@pytest.mark.parametrize('D', [200, 2048])
def test_gather_scores_within_the_stated_bound(D):
    """|score - fp64 sum| <= (D + 2) 2^-24 sum_k |q_k b_k| (include/dir_engine.h)."""
    from dirtorch_amd import ops
    r = np.random.RandomState(130)
    q, b = synth_descriptors(5, 33, D), synth_descriptors(6, 3000, D)
    cand = _cand(r, 33, 400, 3000)
    want, mass = _gather_ref(q, b, cand)
    got = ops.gather_scores(_cuda(q), _cuda(b), _cuda(cand, np.int32)).cpu().numpy().astype(np.float64)
    ok = cand >= 0
    assert np.isnan(got[~ok]).all()
    err = np.abs(got - want)[ok] / mass[ok]
    print('D = %d: max error %.3g of sum |q b|, bound %.3g' % (D, err.max(), (D + 2) * 2.0 ** -24))
    assert (err <= (D + 2) * 2.0 ** -24).all()


# ---- Int8Index ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sets():
    """The inputs tests/test_index_cpu.py checks the re-rank condition on, their quantised and exact scores."""
    q, b = synth_descriptors(5, 33, 200), synth_descriptors(6, 3000, 200)
    quant = index_ref.score(*index_ref.quantize(q), *index_ref.quantize(b))
    exact64 = q.astype(np.float64) @ b.astype(np.float64).T
    mass = np.abs(q.astype(np.float64)) @ np.abs(b.astype(np.float64)).T            # sum_k |q_k b_k|
    return dict(q=q, b=b, quant=quant, exact64=exact64, exact=exact64.astype(np.float32), mass=mass)


def _index(b):
    from dirtorch_amd.index import Int8Index
    return Int8Index(b.shape[1]).add(b)


def test_search_by_quantised_score(sets):
    """The lists are topk_ref of the restatement's scores, value bits included, whatever the chunking and however the
    database was added."""
    from dirtorch_amd.index import Int8Index
    q, b = sets['q'], sets['b']
    one = _index(b)
    three = Int8Index(200)
    three.add(b[:1000])                                           # an ndarray,
    three.add(torch.from_numpy(b[1000:1001]))                     # a CPU tensor,
    three.add(torch.from_numpy(b[1001:]).cuda())                  # a CUDA tensor
    assert len(one) == len(three) == 3000
    assert torch.equal(one.codes, three.codes) and torch.equal(one.scales, three.scales)
    wc, ws = index_ref.quantize(b)
    assert (one.codes.cpu().numpy() == wc).all() and (bits(one.scales.cpu().numpy()) == bits(ws)).all()
    for k in (10, 100):
        want = topk_ref_rows(sets['quant'], k)
        for index in (one, three):
            for kw in ({}, dict(scratch_bytes=4 * 3000 * 10), dict(db_rows=701), dict(db_rows=701, scratch_bytes=4 * 701 * 10)):
                idx, vals = index.search(q, k, **kw)
                assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
                _same((idx, vals), want, '%r, k = %d' % (kw, k))


def test_search_same_set_and_short_rows(sets):
    b = sets['b'][:600]
    index = _index(b)
    quant = index_ref.score(*index_ref.quantize(b), *index_ref.quantize(b))
    own = np.arange(600, dtype=np.int32)
    for k, kw in ((20, {}), (20, dict(db_rows=177, scratch_bytes=4 * 177 * 250)), (600, {})):
        idx, vals = index.search(b, k, same_set=True, **kw)
        _same((idx, vals), topk_ref_rows(quant, k, exclude=own), 'k = %d' % k)
        assert (idx.cpu().numpy() != own[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours
    idx, vals = index.search(b, 600, rerank=600, source=_cuda(b), same_set=True)
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all() and (idx[:, :-1] >= 0).all()


def test_search_rerank_gives_the_exact_lists(sets, tmp_path):
    """(k, R) = (10, 40) and (100, 400): the indices are topk_ref of the exact scores (tests/test_index_cpu.py holds the
    condition for the restatement), the values within gather_scores' bound of the fp64 scores; a host memmap as the
    source gives the CUDA source's result bit for bit."""
    q, b = sets['q'], sets['b']
    index = _index(b)
    np.save(str(tmp_path / 'b.npy'), b)
    mm = np.load(str(tmp_path / 'b.npy'), mmap_mode='r')
    rows = np.arange(33)[:, None]
    for k, R in ((10, 40), (100, 400)):
        idx, vals = index.search(q, k, rerank=R, source=_cuda(b))
        want = topk_ref_rows(sets['exact'], k)[0]
        got = idx.cpu().numpy()
        print('k = %d, R = %d: %d of 33 lists equal the exact lists' % (k, R, int((got == want).all(axis=1).sum())))
        assert (got == want).all()
        err = np.abs(vals.cpu().numpy().astype(np.float64) - sets['exact64'][rows, got])
        assert (err <= 202 * 2.0 ** -24 * sets['mass'][rows, got]).all()
        for kw in ({}, dict(scratch_bytes=4 * R * 200 * 5), dict(db_rows=701)):
            idx2, vals2 = index.search(q, k, rerank=R, source=mm, **kw)
            assert torch.equal(idx2, idx) and torch.equal(vals2.view(torch.int32), vals.view(torch.int32)), kw
        idx2, vals2 = index.search(q, k, rerank=R, source=torch.from_numpy(b))
        assert torch.equal(idx2, idx) and torch.equal(vals2.view(torch.int32), vals.view(torch.int32))


def test_search_rerank_exact_on_small_integers():
    """Operands in [-3, 3]: the re-scored values are exact, so lists and value bits equal the fp64 reference - the k best,
    by exact score, of the restatement's shortlist."""
    r = np.random.RandomState(140)
    N, D, k, R = 600, 64, 20, 80
    x = r.randint(-3, 4, (N, D)).astype(np.float32)
    quant = index_ref.score(*index_ref.quantize(x), *index_ref.quantize(x))
    exact = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    own = np.arange(N, dtype=np.int32)
    cand = topk_ref_rows(quant, R, exclude=own)[0]
    want = topk_ref_rows(np.take_along_axis(exact, cand.astype(np.int64), axis=1), k, ids=cand)
    index = _index(x)
    for source in (_cuda(x), x):
        _same(index.search(x, k, rerank=R, source=source, same_set=True), want)
    _same(index.search(x[:50], k, rerank=R, source=_cuda(x), db_rows=177),
          topk_ref_rows(np.take_along_axis(exact[:50], topk_ref_rows(quant[:50], R)[0].astype(np.int64), axis=1), k,
                        ids=topk_ref_rows(quant[:50], R)[0]))


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd import ops
    from dirtorch_amd.index import Int8Index
    q, b = sets['q'], sets['b']
    index = _index(b)
    path = str(tmp_path / 'index.npz')
    index.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'codes', 'scales'] and f['codes'].shape == (3000, 200) and f['codes'].dtype == np.int8
    back = Int8Index.load(path)
    assert back.D == 200 and len(back) == 3000
    assert torch.equal(back.codes, index.codes) and torch.equal(back.scales.view(torch.int32), index.scales.view(torch.int32))
    for kw in (dict(), dict(rerank=40, source=_cuda(b))):
        a, c = index.search(q, 10, **kw), back.search(q, 10, **kw)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1].view(torch.int32), c[1].view(torch.int32))
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=40)                           # no source
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=9, source=b)                  # R < k
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=ops.topk_max_k() + 1, source=b)
    with pytest.raises(ValueError):
        index.search(q, 3001)
    with pytest.raises(ValueError):
        index.search(q, 10, same_set=True)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 199), np.float32))


# ---- python -m dirtorch_amd.retrieve --index int8 ----------------------------------------------------------------------
def test_retrieve_cli_with_an_int8_index(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): with --index int8 --rerank 28 the .npz holds what
    Int8Index.search gives for the same descriptors; without the new flags it still holds retrieve_device's lists."""
    import dir_oracle as O
    from dirtorch_amd import ranking
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
    runs = {'int8': ['--index', 'int8', '--rerank', '28'], 'plain': []}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', outs[name]] + flags, env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    want = _index(x).search(x, k, rerank=28, source=x, same_set=True)
    npz = np.load(outs['int8'])
    assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
    _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in want), 'int8')
    assert (npz['idx'] != np.arange(N)[:, None]).all()
    npz = np.load(outs['plain'])
    _same((npz['idx'], npz['scores']), tuple(t.cpu().numpy() for t in ranking.retrieve_device(x, x, k, same_set=True)), 'plain')

"""The product-quantised index on the device (dir_pq_encode, dir_pq_lut, dir_pq_scan, index.PQIndex, python -m
dirtorch_amd.retrieve --index pq).  Codes, tables and scores are chains of single fp32 operations in a fixed order
(include/dir_engine.h), so everything is compared bit for bit with the numpy restatement of tests/pq_ref.py; a reference is
computed once per shape, at the largest row count, and the smaller cases are compared with its slices (rows and queries
are independent)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pq_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (D, M): the shapes asked for, then sub-spaces wider than the 32 columns staged at a time (dsub = 40: two chunks, the
# second short; dsub = 130: five)
DM = [(8, 1), (12, 3), (64, 8), (200, 8), (2048, 64), (2048, 128), (256, 128), (80, 2), (130, 1)]
ENC_ROWS = 256            # rows of an encoder workgroup (eight passes of 32)


def _same_bits(got, want, what=''):
    """bit for bit; where the reference holds a NaN, a NaN (an x86 host and the device give inf - inf different signs)"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert got.shape == want.shape and ok.all(), (what, np.argwhere(~ok)[:5])


def _codebooks(r, D, M):
    """random centroids; 17 and 250 repeat centroid 3 and centroid 255 repeats 254 in every sub-space (ties)"""
    cb = r.standard_normal((M, 256, D // M)).astype(np.float32)
    cb[:, 17], cb[:, 250], cb[:, 255] = cb[:, 3], cb[:, 3], cb[:, 254]
    return cb


# ---- pq_encode ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,M', DM)
def test_encode_is_the_restatement(D, M):
    """N = 1, 255, 257 (one row past a workgroup's 256) and 32 * 9 + 1 rows: a row that IS centroid 3 / 254 of every
    sub-space (distance 0 three times / twice: the smallest index), a row with a NaN, a row of zeros; rows at a pitch;
    codes at a pitch through the C ABI - the bytes M .. M rounded up to 4 are zero, the bytes past that untouched."""
    from dirtorch_amd import _lib, ops
    r = np.random.RandomState(200 + D + M)
    dsub, N = D // M, ENC_ROWS + 33
    cb = _codebooks(r, D, M)
    x = r.standard_normal((N, D)).astype(np.float32)
    x[11] = cb[:, 3].reshape(-1)
    x[12] = cb[:, 254].reshape(-1)
    x[5, D // 2] = np.nan
    x[9] = 0
    want = pq_ref.encode(x, cb)
    assert (want[11] == 3).all() and (want[12] == 254).all() and want[5, (D // 2) // dsub] == 0
    dcb, dx = _cuda(cb), _cuda(x)
    ldc = (M + 3) // 4 * 4
    for n in (1, 255, ENC_ROWS + 1, N):
        got = ops.pq_encode(dx[:n], dcb)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, ldc) and got.is_cuda
        g = got.cpu().numpy()
        assert (g[:, :M] == want[:n]).all(), (n, np.argwhere(g[:, :M] != want[:n])[:5])
        assert not g[:, M:].any()
    wide = torch.full((N, D + 3), float('nan'), device='cuda')
    wide[:, :D] = dx
    assert (ops.pq_encode(wide[:, :D], dcb).cpu().numpy()[:, :M] == want).all()
    out = torch.full((N, ldc + 8), 0xAB, dtype=torch.uint8, device='cuda')
    _lib.call('dir_pq_encode', _lib.ptr(dx), D, N, D, M, _lib.ptr(dcb), _lib.ptr(out), ldc + 8, _lib.stream_ptr())
    o = out.cpu().numpy()
    assert (o[:, :M] == want).all() and not o[:, M:ldc].any() and (o[:, ldc:] == 0xAB).all()
    assert torch.equal(ops.pq_encode(dx, dcb), ops.pq_encode(dx, dcb))


def test_encode_nan_centroids_never_win():
    from dirtorch_amd import ops
    r = np.random.RandomState(230)
    cb = _codebooks(r, 64, 8)
    cb[0, 0], cb[1, 40], cb[2] = np.nan, np.nan, np.nan
    x = r.standard_normal((70, 64)).astype(np.float32)
    x[3, :8] = cb[0, 1]
    want = pq_ref.encode(x, cb)
    assert (want[:, 0] != 0).all() and (want[:, 1] != 40).all() and not want[:, 2].any()
    assert (ops.pq_encode(_cuda(x), _cuda(cb)).cpu().numpy()[:, :8] == want).all()


# ---- pq_lut ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,M', DM)
def test_lut_is_the_restatement(D, M):
    """Q = 1, 3, 33 (one past a workgroup's 32 queries), 70; queries at a pitch; a zero query gives +0 everywhere."""
    from dirtorch_amd import ops
    r = np.random.RandomState(300 + D + M)
    cb = _codebooks(r, D, M)
    q = (r.standard_normal((70, D)) * np.exp(r.uniform(-2, 2, (70, 1)))).astype(np.float32)
    q[2] = 0
    want = pq_ref.lut(q, cb)
    dcb, dq = _cuda(cb), _cuda(q)
    for n in (1, 3, 33, 70):
        got = ops.pq_lut(dq[:n], dcb)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, M, 256) and got.is_contiguous()
        _same_bits(got, want[:n], 'Q = %d' % n)
    wide = torch.full((70, D + 5), float('nan'), device='cuda')
    wide[:, :D] = dq
    _same_bits(ops.pq_lut(wide[:, :D], dcb), want)
    assert not bits(want[2]).any()


# ---- pq_scan -----------------------------------------------------------------------------------------------------------
def _tile(M):
    """the rows of a scan workgroup"""
    return 2048 if M <= 64 else 1024


FILL = 12345.0


def _scan_case(M, r):
    """(tables [70, M, 256], codes [2 tile + 3, ldc + 4] with noise in the padding, the restatement's scores): tables over
    a wide range of magnitudes with -0.0, +-inf and NaN entries (some scores are +-inf, some NaN)"""
    t = (r.standard_normal((70, M, 256)) * np.exp(r.uniform(-6, 6, (70, M, 1)))).astype(np.float32)
    flat = t.reshape(-1)
    n = flat.size
    flat[r.randint(0, n, n // 50)] = -0.0
    flat[r.randint(0, n, max(n // 3000, 3))] = np.inf
    flat[r.randint(0, n, max(n // 3000, 3))] = -np.inf
    flat[r.randint(0, n, max(n // 5000, 2))] = np.nan
    t[1] = -0.0                                           # every entry -0: the score is +0 (the chain starts at +0)
    N = 2 * _tile(M) + 3
    codes = r.randint(0, 256, (N, (M + 3) // 4 * 4 + 4)).astype(np.uint8)
    return t, codes, pq_ref.scan(t, codes[:, :M])


def _check_scan(dt, dc, want, Q, N, past=5):
    """one ops.pq_scan call into a buffer `past` columns wider than N: the scores' bits, nothing written past N"""
    from dirtorch_amd import ops
    out = torch.full((Q, N + past), FILL, device='cuda')
    got = ops.pq_scan(dt[:Q], dc[:N], out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (Q, N)
    _same_bits(got, want[:Q, :N], 'Q = %d, N = %d' % (Q, N))
    assert (out[:, N:] == FILL).all()
    return got


# the issue's M, and the widths where the kernel changes form: 8 | 9 .. 16 | 17 .. 32 | 33 .. 64 | 65 .. 128
@pytest.mark.parametrize('M', [1, 3, 8, 9, 16, 17, 32, 33, 64, 65, 128])
def test_scan_is_the_restatement(M):
    """N = 1, 255, 256, 257, a tile - 1, a tile, a tile + 1, two tiles + 3 at Q = 70 (workgroups of 8 queries: pairs, and
    at 70 a last workgroup of 6); Q = 1, 2, 3, 7, 33 (a single query, a pair, a pair and a half, ... - every parity of the
    table buffers, and a workgroup left with one query) at a tile + 1 rows."""
    from dirtorch_amd import ops
    r = np.random.RandomState(400 + M)
    t, codes, want = _scan_case(M, r)
    assert np.isnan(want).any() and np.isinf(want).any() and not bits(want[1]).any()
    dt, dc = _cuda(t), _cuda(codes, np.uint8)
    T = _tile(M)
    for N in (1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3):
        _check_scan(dt, dc, want, 70, N)
    for Q in (1, 2, 3, 7, 33):
        _check_scan(dt, dc, want, Q, T + 1)
    a, b = ops.pq_scan(dt, dc), ops.pq_scan(dt, dc)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # codes without a pitch (ldc = M: copied to a multiple of 4 where it is none)
    _same_bits(ops.pq_scan(dt[:5], dc[:300, :M].contiguous()), want[:5, :300])


@pytest.mark.parametrize('M', [8, 64, 128])
@pytest.mark.parametrize('value', [0, 255])
def test_scan_of_equal_codes(M, value):
    """every code 0 / 255: all lanes read one entry of every table (its first / last)"""
    r = np.random.RandomState(450 + M)
    t = r.standard_normal((3, M, 256)).astype(np.float32)
    N = _tile(M) + 1
    codes = np.full((N, M), value, np.uint8)
    _check_scan(_cuda(t), _cuda(codes, np.uint8), pq_ref.scan(t, codes), 3, N)


# ---- PQIndex -----------------------------------------------------------------------------------------------------------
PD, PM = 64, 8


@pytest.fixture(scope='module')
def sets():
    """33 queries, 3000 clustered rows of 64 values, an index of 8 sub-spaces trained on the rows and its codebooks on the
    host; the restatement's scores of the queries (every list below is a top-k of them)."""
    from dirtorch_amd.index import PQIndex
    q, b = synth_descriptors(5, 33, PD), synth_descriptors(6, 3000, PD)
    index = PQIndex(PD, PM).train(b, iters=10, seed=0).add(b)
    cb = index.codebooks.cpu().numpy()
    return dict(q=q, b=b, index=index, cb=cb, codes=pq_ref.encode(b, cb))


def test_search_is_the_restatement(sets):
    q, b, index = sets['q'], sets['b'], sets['index']
    assert len(index) == 3000 and index.M == PM and index.nbytes() == 3000 * PM
    assert (index.codes.cpu().numpy()[:, :PM] == sets['codes']).all()
    for k in (1, 10, 100):
        want = pq_ref.search_ref(q, b, sets['cb'], k)
        idx, vals = index.search(q, k)
        assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
        _same((idx, vals), want, 'k = %d' % k)
        _same(index.search(_cuda(q), k, db_rows=700), want, 'db_rows, k = %d' % k)
        # 4 * 3000 bytes of scores and 1024 * 8 bytes of tables per query: 11 queries a chunk, three chunks
        _same(index.search(q, k, scratch_bytes=11 * (4 * 3000 + 1024 * PM)), want, 'scratch_bytes, k = %d' % k)
        _same(index.search(q, k, db_rows=700, scratch_bytes=11 * (4 * 700 + 1024 * PM)), want, 'both, k = %d' % k)


def test_the_index_does_not_depend_on_the_add_calls(sets):
    from dirtorch_amd.index import PQIndex
    q, b, one = sets['q'], sets['b'], sets['index']
    for parts in ((b[:1000], b[1000:1001], b[1001:]),
                  (b[:1000], torch.from_numpy(b[1000:1001]), torch.from_numpy(b[1001:]).cuda())):
        index = PQIndex(PD, PM)
        index.codebooks = one.codebooks.clone()
        for part in parts:
            index.add(part)
        assert len(index) == 3000 and torch.equal(index.codes, one.codes)
        _same(index.search(q, 10), one.search(q, 10))


def test_same_set_and_short_rows(sets):
    from dirtorch_amd.index import PQIndex
    b = sets['b'][:600]
    index = PQIndex(PD, PM).train(b, iters=2).add(b)
    own = np.arange(600, dtype=np.int32)
    cb = index.codebooks.cpu().numpy()
    for k, kw in ((20, {}), (20, dict(db_rows=250)), (600, {})):
        idx, vals = index.search(b, k, same_set=True, **kw)
        _same((idx, vals), pq_ref.search_ref(b, b, cb, k, exclude=own), 'k = %d, %r' % (k, kw))
        assert (idx.cpu().numpy() != own[:, None]).all()
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()        # k = N: a row has N - 1 neighbours


def test_rerank_with_a_device_and_a_host_source(sets, tmp_path):
    """rerank = R: the restatement's R best, re-scored by ops.gather_scores against the fp32 rows and ranked again; a host
    ndarray and a memmap give the CUDA source's result bit for bit."""
    from dirtorch_amd import ops
    q, b, index = sets['q'], sets['b'], sets['index']
    np.save(str(tmp_path / 'b.npy'), b)
    mm = np.load(str(tmp_path / 'b.npy'), mmap_mode='r')
    for k, R in ((10, 40), (100, 400)):
        cand = _cuda(pq_ref.search_ref(q, b, sets['cb'], R)[0], np.int32)
        want = ops.topk(ops.gather_scores(_cuda(q), _cuda(b), cand), k, ids=cand)
        _same(index.search(q, k, rerank=R, source=_cuda(b)), want, 'device source, R = %d' % R)
        _same(index.search(q, k, rerank=R, source=b, scratch_bytes=11 * (4 * 3000 + 1024 * PM)), want, 'host source')
        _same(index.search(q, k, rerank=R, source=mm), want, 'memmap source')


def test_save_load_round_trip_and_argument_errors(sets, tmp_path):
    from dirtorch_amd.index import PQIndex
    q, b, index = sets['q'], sets['b'], sets['index']
    path = str(tmp_path / 'pq.npz')
    index.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['D', 'M', 'codebooks', 'codes']
        assert f['codes'].shape == (3000, PM) and f['codes'].dtype == np.uint8
        assert f['codebooks'].shape == (PM, 256, PD // PM) and f['codebooks'].dtype == np.float32
        saved = {name: f[name] for name in f.files}
    back = PQIndex.load(path)
    assert back.D == PD and back.M == PM and len(back) == 3000 and torch.equal(back.codes, index.codes)
    assert torch.equal(back.codebooks.view(torch.int32), index.codebooks.view(torch.int32))
    for kw in ({}, dict(rerank=40, source=_cuda(b))):
        _same(back.search(q, 10, **kw), index.search(q, 10, **kw))
    for bad in (dict(codes=saved['codes'].astype(np.int8)), dict(codes=saved['codes'][:, :PM - 1]),
                dict(codebooks=saved['codebooks'][:, :255]), dict(codebooks=saved['codebooks'][:PM - 1]), dict(M=np.int64(7))):
        np.savez(str(tmp_path / 'bad.npz'), **dict(saved, **bad))
        with pytest.raises(ValueError):
            PQIndex.load(str(tmp_path / 'bad.npz'))
    for D, M in ((64, 0), (64, 7), (64, 129), (0, 1), (256, 256)):
        with pytest.raises(ValueError):
            PQIndex(D, M)
    fresh = PQIndex(PD, PM)
    with pytest.raises(ValueError):
        fresh.search(q, 10)                                      # before train
    with pytest.raises(ValueError):
        fresh.add(b)                                             # before train
    with pytest.raises(ValueError):
        fresh.save(path)
    with pytest.raises(ValueError):
        fresh.train(b[:255])                                     # fewer rows than centroids
    with pytest.raises(ValueError):
        fresh.train(b, max_rows=100)
    bad = b[:300].copy()
    bad[17, 3] = np.inf
    with pytest.raises(ValueError):
        fresh.train(bad)
    with pytest.raises(ValueError):
        index.train(b)                                           # after add
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=40)                           # no source
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=9, source=b)                  # R < k
    with pytest.raises(ValueError):
        index.search(q, 10, rerank=40, source=b[:100])
    with pytest.raises(ValueError):
        index.search(q, 3001)
    with pytest.raises(ValueError):
        index.search(q, 0)
    with pytest.raises(ValueError):
        index.search(q, 10, same_set=True)                       # 33 queries, 3000 rows
    with pytest.raises(ValueError):
        index.search(q[:, :63], 10)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 63), np.float32))
    idx, vals = index.search(q[:0], 10)
    assert tuple(idx.shape) == (0, 10) and tuple(vals.shape) == (0, 10)


def test_training_is_reproducible_and_reduces_the_error(sets):
    """Two runs from one seed: identical bits, from host rows and from device rows.  The mean squared reconstruction error
    of the training rows (fp64 on the host, from ops.pq_encode's codes) is strictly below that of the initial codebooks
    (iters = 0), which are rows of the sample.  A sample (more rows than max_rows) is the sorted RandomState choice."""
    from dirtorch_amd import ops
    from dirtorch_amd.index import PQIndex
    b, index = sets['b'], sets['index']
    again = PQIndex(PD, PM).train(_cuda(b), iters=10, seed=0)
    assert torch.equal(again.codebooks.view(torch.int32), index.codebooks.view(torch.int32))
    start = PQIndex(PD, PM).train(b, iters=0, seed=0)
    first = np.sort(np.random.RandomState(0).choice(3000, 256, replace=False))
    assert (bits(start.codebooks.cpu().numpy()) == bits(b[first].reshape(256, PM, PD // PM).transpose(1, 0, 2))).all()
    errs = []
    for ix in (start, index):
        cb = ix.codebooks.cpu().numpy()
        codes = ops.pq_encode(_cuda(b), ix.codebooks).cpu().numpy()[:, :PM]
        errs.append(pq_ref.reconstruction_error(b, cb, codes))
    print('reconstruction error %.6f with the initial codebooks, %.6f after 10 iterations' % tuple(errs))
    assert np.isfinite(errs).all() and errs[1] < errs[0]
    small = PQIndex(PD, PM).train(b, iters=2, seed=3, max_rows=500)
    pick = np.sort(np.random.RandomState(3).choice(3000, 500, replace=False))
    same = PQIndex(PD, PM).train(b[pick], iters=2, seed=3)
    assert torch.equal(small.codebooks.view(torch.int32), same.codebooks.view(torch.int32))


# ---- python -m dirtorch_amd.retrieve --index pq ------------------------------------------------------------------------
def test_retrieve_cli_with_a_product_quantiser(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): the .npz of --index pq --pq-m 8, without and with
    --rerank, equals PQIndex.search on the same descriptors; an M that does not divide the width ends the run."""
    import dir_oracle as O
    from dirtorch_amd import retrieve
    from dirtorch_amd.index import PQIndex
    r = np.random.RandomState(71)
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
    runs = {'raw': ['--index', 'pq', '--pq-m', '8'], 'rerank': ['--index', 'pq', '--pq-m', '8', '--rerank', '28'],
            'odd': ['--index', 'pq', '--pq-m', '5']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = {name: subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve'] + base + ['--output', outs[name]] + flags,
                                    env=env) for name, flags in runs.items()}
    codes = {name: p.wait(timeout=300) for name, p in procs.items()}
    assert codes['raw'] == 0 and codes['rerank'] == 0 and codes['odd'] != 0 and not os.path.exists(outs['odd'])
    index = PQIndex(D, 8).train(x).add(x)
    for name, kw in (('raw', {}), ('rerank', dict(rerank=28, source=x))):
        got = np.load(outs[name])
        assert sorted(got.files) == ['idx', 'scores'] and got['idx'].dtype == np.int32 and got['scores'].dtype == np.float32
        _same((got['idx'], got['scores']), index.search(x, k, same_set=True, **kw), name)
        assert (got['idx'] != np.arange(N)[:, None]).all() and (got['idx'] >= 0).all()
    with pytest.raises(SystemExit, match='pq-m'):
        retrieve.main(base + ['--output', outs['odd'], '--index', 'pq'])          # no --pq-m: before anything is loaded

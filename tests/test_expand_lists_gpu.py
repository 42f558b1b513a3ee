"""alpha-QE / DBA from neighbour lists on the device (dir_expand_lists, ops.expand_lists, ranking.expand_device, the
--expand flag of python -m dirtorch_amd.retrieve, eval_dir.eval_model(expand=)) against the numpy restatement of tests/expand_ref.py.  The definition is
a chain of single fp32 operations, so with an integer alpha the device's rows are compared bit for bit; only powf (a
non-integer alpha) and the comparison with the matrix route have bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from expand_ref import expand_lists_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from test_oracle_golden import QE_CASES, qe_inputs
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, M_ROWS = 37, 53
NAN_ROW = 5      # make_lists: the row that carries a NaN weight on a valid id


def make_lists(n, m, k, seed):
    """(idx [n,k] int32, vals [n,k] float32): random ids and scores of both signs, and - where k has room - row 1 with an
    empty slot at the end, row 2 with one in the middle, row 3 with a repeated id, row 4 empty throughout (the vals of every
    empty slot NaN: they must not be read), row NAN_ROW with a NaN score on a valid id."""
    r = np.random.RandomState(seed)
    idx = r.randint(0, m, (n, k)).astype(np.int32)
    vals = r.uniform(-1, 1, (n, k)).astype(np.float32)
    if k >= 1:
        idx[1, -1] = -1
        idx[4, :] = -1
        vals[NAN_ROW, 0] = np.nan
    if k >= 4:
        idx[2, 1] = -1
        idx[3, 2] = idx[3, 0]
    vals[idx < 0] = np.nan
    return idx, vals


def _wide(a, pad, fill):
    """a [rows, w] -> a CUDA buffer [rows, w + pad] holding it, `fill` in the padding"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    out = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out.cuda()


def run_kernel(descs, db, idx, vals, alpha, pad):
    """the rows of dir_expand_lists as an ndarray.  pad = 0: through ops.expand_lists on contiguous tensors; else through
    the C ABI with every pitch = width + pad - NaN in the padding of the fp32 operands, an id far outside the database in
    that of idx - and the padding of out must come back untouched."""
    from dirtorch_amd import _lib, ops
    if pad == 0:
        out = ops.expand_lists(_cuda(descs), _cuda(db), _cuda(idx, np.int32), _cuda(vals), alpha)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == descs.shape and out.is_contiguous()
        return out.cpu().numpy()
    (n, D), m, k = descs.shape, db.shape[0], idx.shape[1]
    wd, wb = _wide(descs, pad, float('nan')), _wide(db, pad, float('nan'))
    wi, wv = _wide(idx, pad, 1 << 30), _wide(vals, pad, float('nan'))
    wo = torch.full((n, D + pad), 7.0, dtype=torch.float32, device='cuda')
    _lib.call('dir_expand_lists', _lib.ptr(wd), D + pad, n, _lib.ptr(wb), D + pad, m, D, _lib.ptr(wi), _lib.ptr(wv), k + pad, k,
              float(alpha), _lib.ptr(wo), D + pad, _lib.stream_ptr())
    got = wo.cpu().numpy()
    assert (got[:, D:] == 7.0).all(), 'the padding of out was written'
    return np.ascontiguousarray(got[:, :D])


def assert_same_rows(got, want, nan_rows, what):
    """equal stored bits; a row of `nan_rows` is NaN throughout in both (which NaN an operation returns is not part of the
    definition) and no other row holds one"""
    nan = np.zeros(len(want), bool)
    nan[np.asarray(list(nan_rows), dtype=np.int64)] = True
    assert np.isnan(want[nan]).all() and not np.isnan(want[~nan]).any(), what
    assert np.isnan(got[nan]).all(), what
    assert torch.equal(torch.from_numpy(bits(got[~nan]).astype(np.int64)), torch.from_numpy(bits(want[~nan]).astype(np.int64))), (
        what, np.argwhere(bits(got[~nan]) != bits(want[~nan]))[:5])


# ---- the kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 3, 4, 255, 256, 1028, 2048, 2052])
def test_kernel_bit_for_bit(D):
    """dir_expand_lists against expand_lists_ref, bit for bit, n = 37 rows against m = 53: D below one lane's four columns,
    with a scalar tail, below / at one span of 1024, with a ragged second span, at two spans (the widest the sums wait in
    registers for) and past them; k = 0 (normalise only), 1, 4, 5, 9 - at and across the unroll of four; alpha = 0, 1, 3
    on scores of both signs; contiguous operands (16-byte loads when D % 4 == 0), pitches of width + 4 (the same loads
    at a pitch) and width + 3 (unaligned rows: the scalar path); empty slots at the end, in the middle and throughout
    with NaN in their vals, a repeated id, and a NaN weight that must stay in its row."""
    r = np.random.RandomState(100 + D)
    descs = r.standard_normal((N_ROWS, D)).astype(np.float32)
    db = r.standard_normal((M_ROWS, D)).astype(np.float32)
    for k in (0, 1, 4, 5, 9):
        idx, vals = make_lists(N_ROWS, M_ROWS, k, 7 * D + k)
        for alpha in (0, 1, 3):
            want = expand_lists_ref(descs, db, idx, vals, alpha)
            nan_rows = [NAN_ROW] if k >= 1 and alpha > 0 else []      # (v^0 is 1 for a NaN too: zero multiplications)
            for pad in (0, 3, 4):
                got = run_kernel(descs, db, idx, vals, alpha, pad)
                assert_same_rows(got, want, nan_rows, 'D %d k %d alpha %d pad %d' % (D, k, alpha, pad))


def test_self_set_reads_the_rows_it_is_given():
    """db IS descs (the DBA form: one buffer for both operands) gives what two copies give."""
    from dirtorch_amd import ops
    r = np.random.RandomState(3)
    x = r.standard_normal((M_ROWS, 260)).astype(np.float32)
    idx, vals = make_lists(M_ROWS, M_ROWS, 6, 11)
    dev = _cuda(x)
    got = ops.expand_lists(dev, dev, _cuda(idx, np.int32), _cuda(vals), 3).cpu().numpy()
    assert_same_rows(got, expand_lists_ref(x, x, idx, vals, 3), [NAN_ROW], 'self')
    assert torch.equal(dev.cpu(), torch.from_numpy(x))


def test_non_integer_alpha_within_powf():
    """alpha = 0.5 on positive scores against the restatement in float64 at rtol 1e-6.  powf is the one step that is not
    bit-defined; the rest of the fp32 chain has to fit the same bound, so the inputs keep it free of cancellation:
    every descriptor entry is positive (all k + 1 terms of a sum have one sign) and D = 256 gives a lane one column.  Worst
    case in units of 2^-24 = 6e-8: the weight 2 (powf), the product 1, k = 4 sums 4, the mean 1, the sum of squares (1
    product + 8 tree sums) / 2 = 4.5 after the root, the root and the division 2 - 14.5, or 8.7e-7."""
    r = np.random.RandomState(17)
    D, k = 256, 4
    descs = np.abs(r.standard_normal((N_ROWS, D))).astype(np.float32) + np.float32(0.1)
    db = np.abs(r.standard_normal((M_ROWS, D))).astype(np.float32) + np.float32(0.1)
    idx = r.randint(0, M_ROWS, (N_ROWS, k)).astype(np.int32)
    vals = r.uniform(0.05, 1, (N_ROWS, k)).astype(np.float32)
    idx[1, -1] = -1
    vals[1, -1] = np.nan
    want = expand_lists_ref(descs, db, idx, vals, 0.5, dtype=np.float64)
    for pad in (0, 3):
        got = run_kernel(descs, db, idx, vals, 0.5, pad).astype(np.float64)
        print('alpha 0.5, pad %d: largest relative error %.3g' % (pad, np.abs(got / want - 1).max()))
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)


def test_errors_and_empty_calls():
    """The DIR_ERR_INVALID cases of the header raise with device operands as they do with host ones (nothing is launched),
    n == 0 returns an empty tensor, and ops checks what the C ABI cannot see."""
    from dirtorch_amd import _lib, ops
    n, m, D, k = 4, 6, 8, 3
    x, b = torch.zeros(n, D, device='cuda'), torch.zeros(m, D, device='cuda')
    idx, vals = torch.zeros(n, k, dtype=torch.int32, device='cuda'), torch.zeros(n, k, device='cuda')
    out = torch.empty(n, D, device='cuda')

    def call(descs=x, ldd=D, n=n, db=b, ldb=D, m=m, D=D, idx=idx, vals=vals, ldl=k, k=k, alpha=1.0, out=out, ldo=D):
        _lib.call('dir_expand_lists', _lib.ptr(descs), ldd, n, _lib.ptr(db), ldb, m, D, _lib.ptr(idx), _lib.ptr(vals), ldl, k,
                  alpha, _lib.ptr(out), ldo, _lib.stream_ptr())

    call()
    for bad in (dict(n=-1), dict(m=-1), dict(k=-1), dict(D=0), dict(ldd=D - 1), dict(ldb=D - 1), dict(ldo=D - 1),
                dict(ldl=k - 1), dict(alpha=-1.0), dict(descs=None), dict(db=None), dict(idx=None), dict(vals=None),
                dict(out=None)):
        with pytest.raises(_lib.DirError) as e:
            call(**bad)
        assert e.value.code == -1, bad
    call(n=0, descs=None, out=None)
    with pytest.raises(_lib.DirError):
        ops.expand_lists(x, b, idx, vals, -2)
    empty = ops.expand_lists(x[:0], b, idx[:0], vals[:0], 1)
    assert tuple(empty.shape) == (0, D) and empty.is_cuda and empty.dtype == torch.float32
    with pytest.raises(TypeError):
        ops.expand_lists(x, b, idx.long(), vals, 1)
    with pytest.raises(ValueError):
        ops.expand_lists(x, b[:, :4], idx, vals, 1)
    with pytest.raises(ValueError):
        ops.expand_lists(x, b, idx[:2], vals, 1)
    with pytest.raises(ValueError):
        ops.expand_lists(x.cpu(), b, idx, vals, 1)


# ---- ranking.expand_device ---------------------------------------------------------------------------------------------
K_ROUTE, ALPHA_ROUTE = 5, 3


@pytest.fixture(scope='module')
def route_sets():
    """(q [40,64], db [300,64]) synthetic descriptors and the four index classes filled with db"""
    from dirtorch_amd.index import Int8Index, IVFInt8Index, IVFPQIndex, PQIndex
    q, db = synth_descriptors(41, 40, 64), synth_descriptors(42, 300, 64)
    indexes = {'int8': (Int8Index(64).add(db), {}),
               'ivf': (IVFInt8Index(64, 8).train(db).add(db), dict(nprobe=3)),
               'pq': (PQIndex(64, 8).train(db).add(db), {}),
               'ivfpq': (IVFPQIndex(64, 4, 8).train(db).add(db), dict(nprobe=2))}
    return q, db, indexes


def _check_route(descs, db, lists, got, alpha):
    """got = expand_lists_ref on the lists the list maker returned, bit for bit"""
    idx, vals = (t.cpu().numpy() for t in lists)
    pool_ = descs if db is None else db
    want = expand_lists_ref(descs, pool_, idx, vals, alpha)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == descs.shape
    assert_same_rows(got.cpu().numpy(), want, [], 'route')
    return idx


def test_expand_device_exact_lists(route_sets):
    from dirtorch_amd import ranking
    q, db, _ = route_sets
    got = ranking.expand_device(q, db=db, alpha=ALPHA_ROUTE, k=K_ROUTE)
    _check_route(q, db, ranking.retrieve_device(q, db, K_ROUTE), got, ALPHA_ROUTE)
    got = ranking.expand_device(db, alpha=ALPHA_ROUTE, k=K_ROUTE)
    idx = _check_route(db, None, ranking.retrieve_device(db, db, K_ROUTE, same_set=True), got, ALPHA_ROUTE)
    assert (idx != np.arange(len(db))[:, None]).all() and (idx >= 0).all()
    assert ranking.expand_device(q, db=db, alpha=ALPHA_ROUTE, k=0) is q
    with pytest.raises(ValueError):
        ranking.expand_device(q, db=db, alpha=1, k=301)           # the list makers' k <= min(m, topk_max_k())
    with pytest.raises(TypeError):
        ranking.expand_device(q, db=db, alpha=1, k=2, nprobe=2)   # search keywords without an index


@pytest.mark.parametrize('rerank', [0, 24])
@pytest.mark.parametrize('kind', ['int8', 'ivf', 'pq', 'ivfpq'])
def test_expand_device_through_an_index(route_sets, kind, rerank):
    """Both forms through each index class, without and with a re-rank: the output is expand_lists_ref of the lists the
    same index.search call returns, bit for bit; a self-set list never holds its own row."""
    from dirtorch_amd import ranking
    q, db, indexes = route_sets
    index, kw = indexes[kind]
    kw = dict(kw, rerank=rerank)
    src = dict(source=db) if rerank else {}
    got = ranking.expand_device(q, db=db, alpha=ALPHA_ROUTE, k=K_ROUTE, index=index, **kw)
    _check_route(q, db, index.search(q, K_ROUTE, **kw, **src), got, ALPHA_ROUTE)
    got = ranking.expand_device(db, alpha=ALPHA_ROUTE, k=K_ROUTE, index=index, **kw)
    idx = _check_route(db, None, index.search(db, K_ROUTE, same_set=True, **kw, **src), got, ALPHA_ROUTE)
    assert (idx != np.arange(len(db))[:, None]).all()


def test_expand_device_short_lists_and_index_checks(route_sets):
    """One probed list of eight cannot fill k = 48 for every row (300 rows: a list holds 37.5 on average), so the -1 rule
    runs end to end; an index of another size or width is refused."""
    from dirtorch_amd import ranking
    from dirtorch_amd.index import Int8Index
    q, db, indexes = route_sets
    index = indexes['ivf'][0]
    got = ranking.expand_device(db, alpha=1, k=48, index=index, nprobe=1)
    idx = _check_route(db, None, index.search(db, 48, nprobe=1, same_set=True), got, 1)
    assert (idx == -1).any() and (idx != np.arange(len(db))[:, None]).all()
    with pytest.raises(ValueError):
        ranking.expand_device(q, db=db[:200], alpha=1, k=3, index=index)
    with pytest.raises(ValueError):
        ranking.expand_device(q[:, :32], db=db[:, :32], alpha=1, k=3, index=Int8Index(32).add(np.ascontiguousarray(db[:299, :32])))


@pytest.mark.parametrize('k,alpha', QE_CASES)
def test_expand_device_against_the_reference_goldens(k, alpha, qe_goldens):
    """exact lists, both forms, against the reference's expand_descriptors outputs at test_ranking_gpu.py's atol"""
    from dirtorch_amd import ranking
    q, db = qe_inputs()
    got_db = ranking.expand_device(q, db=db, alpha=alpha, k=k).cpu().numpy()
    got_self = ranking.expand_device(db, alpha=alpha, k=k).cpu().numpy()
    np.testing.assert_allclose(got_db, qe_goldens['qe.db.k%d.a%d' % (k, alpha)], rtol=0, atol=2e-6)
    np.testing.assert_allclose(got_self, qe_goldens['qe.self.k%d.a%d' % (k, alpha)], rtol=0, atol=2e-6)


# ---- the matrix route against the list route ---------------------------------------------------------------------------
def planted_sets(seed, groups, D, nq):
    """(q [nq,D], db [9 * groups, D]) unit rows with planted neighbours: a group is a centre c and nine rows c + t_s e_s
    over orthonormal (c, e_0 .. e_8, e_q), t_s = 0.3 + 0.05 s, so the scores inside a group, 1 / sqrt((1 + t_s^2)(1 +
    t_s'^2)), lie 1e-2 apart and far above those between groups; a query is c + t e_q of a random group; a little noise
    on everything, the database rows shuffled."""
    g = np.random.RandomState(seed)
    G = 9
    t = 0.3 + 0.05 * np.arange(G + 1)
    bases, db = [], []
    for _ in range(groups):
        basis, _r = np.linalg.qr(g.standard_normal((D, G + 2)))
        bases.append(basis.T)
        db.append(basis[:, 0][None, :] + t[:G, None] * basis[:, 1:G + 1].T)
    db = np.concatenate(db)
    q = []
    for _ in range(nq):
        b = bases[g.randint(groups)]
        q.append(b[0] + t[g.randint(G + 1)] * b[G + 1])
    q = np.stack(q)
    db = db + 0.05 * g.standard_normal(db.shape) / np.sqrt(D)
    q = q + 0.05 * g.standard_normal(q.shape) / np.sqrt(D)
    db /= np.linalg.norm(db, axis=1, keepdims=True)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32), db[g.permutation(len(db))].astype(np.float32)


def test_list_route_against_the_matrix_route():
    """200 queries x 900 rows x 256 columns, k = 7, alpha = 2, the db form and the self-set: where the neighbours are not
    in doubt the two routes give the same rows, 1 - cos < 1e-6 (test_ranking_gpu.py's bound for this operation).  Not in
    doubt, asserted in fp64 for EVERY row: the k-th and the (k + 1)-th score are at least 1e-4 apart, and in the
    self-set all k picks score above 0 (so the matrix route's zeroed diagonal is never picked)."""
    import dir_oracle as O
    from dirtorch_amd import ops, ranking
    k, alpha = 7, 2
    q, db = planted_sets(0, 100, 256, 200)
    assert q.shape == (200, 256) and db.shape == (900, 256)
    for descs, same in ((q, False), (db, True)):
        s = descs.astype(np.float64) @ db.astype(np.float64).T
        if same:
            np.fill_diagonal(s, -np.inf)
        top = -np.sort(-s, axis=1)[:, :k + 1]
        assert (top[:, k - 1] - top[:, k] >= 1e-4).all()
        assert not same or (top[:, k - 1] > 0).all()
        new = ranking.expand_device(descs, db=None if same else db, alpha=alpha, k=k).cpu().numpy()
        old = ops.expand_descriptors(_cuda(descs), None if same else _cuda(db), alpha=float(alpha), k=k).cpu().numpy()
        miss = 1 - O.cosine(new, old)
        print('%s: largest 1 - cos %.3g' % ('self-set' if same else 'db form', miss.max()))
        assert (miss < 1e-6).all()


# ---- python -m dirtorch_amd.retrieve --expand lists ----------------------------------------------------------------------
def test_retrieve_cli_expand_lists(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats) with --adba 4 1 --aqe 3 2: --expand lists writes
    what retrieve_device gives on descriptors expanded with expand_device - exact lists without --index; with --index int8
    --rerank 28 the DBA lists from an index over the un-augmented database, the QE lists from the index over the augmented
    one that also serves the final search - and without --expand the .npz is today's: the matrix route's."""
    import dir_oracle as O
    from dirtorch_amd import ranking, test_dir
    from dirtorch_amd.index import Int8Index
    N, D, k = 120, 32, 7
    x = synth_descriptors(51, N, D)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + key: v for key, v in sd.items()}}, str(tmp_path / 'ck.pt'))
    pkg = os.path.join(ROOT, 'deep-image-retrieval_amd')
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    base = ['--dataset', 'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
            str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0', '--topk', str(k),
            '--adba', '4', '1', '--aqe', '3', '2']
    runs = {'lists': ['--expand', 'lists'], 'int8': ['--expand', 'lists', '--index', 'int8', '--rerank', '28'], 'matrix': []}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve'] + base + ['--output', outs[name]] + flags,
                              env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0, 0]

    def check(name, want):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), want, name)

    b = ranking.expand_device(x, alpha=1, k=4)
    qx = ranking.expand_device(x, db=b, alpha=2, k=3)
    check('lists', ranking.retrieve_device(qx, b, k, same_set=True))
    b = ranking.expand_device(x, alpha=1, k=4, index=Int8Index(D).add(x), rerank=28)
    over_b = Int8Index(D).add(b)
    qx = ranking.expand_device(x, db=b, alpha=2, k=3, index=over_b, rerank=28)
    check('int8', over_b.search(qx, k, rerank=28, source=b, same_set=True))
    b = test_dir.expand_descriptors(x, alpha=1, k=4)
    qx = test_dir.expand_descriptors(x, db=b, alpha=2, k=3)
    check('matrix', ranking.retrieve_device(qx, b, k, same_set=True))


# ---- eval_dir: the device route of a class-labelled dataset ------------------------------------------------------------
def test_eval_dir_expand_lists(tmp_path, monkeypatch):
    """eval_dir.eval_model(expand='lists') under DIRTORCH_AMD_DEVICE_RANK=1 gives what eval_labelled_device gives on
    descriptors expanded with expand_device; where test_dir.eval_model would take over (the switch off) it raises
    instead of quietly expanding through the matrix."""
    from dirtorch_amd import datasets, eval_dir, ranking
    N, D = 120, 32
    x = synth_descriptors(52, N, D)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    db = datasets.ImageListLabels(str(tmp_path / 'db.txt'), root=str(tmp_path))
    qe = dict(adba=dict(k=4, alpha=1), aqe=dict(k=3, alpha=2))
    monkeypatch.setenv('DIRTORCH_AMD_DEVICE_RANK', '1')
    res = eval_dir.eval_model(db, None, '', detailed=True, load_feats=str(tmp_path), expand='lists', **qe)
    b = ranking.expand_device(x, **qe['adba'])
    aps, tops = ranking.eval_labelled_device(db, ranking.expand_device(x, db=b, **qe['aqe']), b)
    assert res['APs'] == [float(a) for a in aps] and res['tops'] == tops
    matrix = eval_dir.eval_model(db, None, '', detailed=True, load_feats=str(tmp_path), **qe)
    print('mAP lists %.6f, matrix %.6f' % (res['mAP'], matrix['mAP']))
    assert list(matrix) == list(res)
    monkeypatch.setenv('DIRTORCH_AMD_DEVICE_RANK', '0')
    with pytest.raises(ValueError, match='lists'):
        eval_dir.eval_model(db, None, '', load_feats=str(tmp_path), expand='lists', **qe)

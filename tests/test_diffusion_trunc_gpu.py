"""Truncated diffusion on the device (dir_diffusion_subgraph, dir_diffusion_solve_local, dir_diffusion_spread,
ranking.diffuse_truncated_device, the --diffusion-trunc flag of python -m dirtorch_amd.retrieve) against the numpy
restatement of tests/diffusion_trunc_ref.py.  The definition is a chain of single fp32 operations in a stated order, so
with an integer gamma everything is compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diffusion_ref import SLAB, exact_lists, mean_ap, planted_lists, solve_ref, two_rings
from diffusion_trunc_ref import solve_local_ref, spread_ref, subgraph_ref
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 1 << 30      # an id in the padding of a table: never to be read
NAN = float('nan')


def assert_bits(got, want, what):
    """equal stored bits, NaNs included (a dead candidate's f is the one NaN pattern of the library's or numpy's making:
    compared as NaN-ness, everything else by bits)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    g, w = np.where(np.isnan(want), np.float32(0), got), np.where(np.isnan(want), np.float32(0), want)
    assert np.array_equal(bits(g), bits(w)), (what, np.argwhere(bits(g) != bits(w))[:5])


def _wide(a, pad, fill):
    """a [.., w] -> a CUDA buffer [.., w + pad] holding it, `fill` in the padding"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    out = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), fill, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out.cuda()


@pytest.fixture(scope='module')
def planted():
    """planted_lists(300, 7) -> dir_knn_graph: (idx, S) as read-only ndarrays"""
    from dirtorch_amd import ops
    idx, vals, _ = planted_lists(300, 7, 23)
    S = ops.knn_graph(_cuda(idx, np.int32), _cuda(vals), 3).cpu().numpy()
    idx.setflags(write=False)
    S.setflags(write=False)
    assert (S != 0).sum() > 1500
    return idx, S


# ---- dir_diffusion_subgraph ----------------------------------------------------------------------------------------------
def candidate_lists(N, Q, T, seed):
    """T distinct rows a query in random order with descending scores, then what a list can hold besides: a -1 hole, an
    id 2^20 past the database (dereferencing it would fault), a later duplicate, and a zero, a negative and a NaN score
    inside the first five slots"""
    r = np.random.RandomState(seed)
    cidx = np.stack([r.permutation(N)[:T] for _ in range(Q)]).astype(np.int32)
    cvals = -np.sort(-r.uniform(0.1, 1.0, (Q, T)).astype(np.float32), axis=1)
    if T >= 37:
        cidx[0, 6], cvals[0, 6] = -1, np.nan
        cidx[-1, 0] = N + (1 << 20)
        cidx[0, 20] = cidx[0, 2]
        cidx[-1, T - 1] = cidx[-1, 1]
        cvals[0, 1], cvals[0, 3], cvals[-1, 4] = 0.0, -0.5, np.nan
    return cidx, cvals


@pytest.mark.parametrize('T', [1, 37, 256, 257, 300])
def test_subgraph_bit_for_bit(planted, T):
    """dir_diffusion_subgraph against subgraph_ref: Q = 1, 3, 70, both seed modes, through ops (packed) and through the raw
    ABI at ldc = T + 2, ldt = T + 3 with the graph at a pitch of k + 3, whose padding must come back untouched"""
    from dirtorch_amd import _lib, ops
    idx, S = planted
    N, k = idx.shape
    gi, gs = _cuda(idx, np.int32), _cuda(S)
    wi, ws = _wide(idx, 3, FAR), _wide(S, 3, NAN)
    for Q in (1, 3, 70):
        cidx, cvals = candidate_lists(N, Q, T, 100 * T + Q)
        for one_hot in (False, True):
            want = subgraph_ref(idx, S, cidx, cvals, 5, 3, one_hot=one_hot)
            what = 'T %d Q %d one_hot %d' % (T, Q, one_hot)
            got = ops.diffusion_subgraph(gi, gs, _cuda(cidx, np.int32), _cuda(cvals), kq=5, gamma=3, one_hot=one_hot)
            assert [tuple(t.shape) for t in got] == [(Q, T), (Q, k, T), (Q, k, T), (Q, T)]
            assert [t.dtype for t in got] == [torch.int32, torch.int32, torch.float32, torch.float32]
            ci, cv = _wide(cidx, 2, FAR), _wide(cvals, 2, NAN)
            ldt = T + 3
            raw = [torch.full((Q, ldt), 7, dtype=torch.int32, device='cuda'), torch.full((Q, k, ldt), 7, dtype=torch.int32, device='cuda'),
                   torch.full((Q, k, ldt), 7.0, device='cuda'), torch.full((Q, ldt), 7.0, device='cuda')]
            _lib.call('dir_diffusion_subgraph', _lib.ptr(wi), k + 3, _lib.ptr(ws), k + 3, N, k, _lib.ptr(ci), _lib.ptr(cv), T + 2, Q, T,
                      5, 3.0, int(one_hot), *[_lib.ptr(t) for t in raw], ldt, _lib.stream_ptr())
            for name, g, r, w in zip(('cid', 'lidx', 'lw', 'y'), got, raw, want):
                r = r.cpu().numpy()
                assert (r[..., T:] == 7).all(), what + ': the padding of %s was written' % name
                for route, arr in (('ops', g.cpu().numpy()), ('abi', r[..., :T])):
                    if arr.dtype == np.float32:
                        assert_bits(arr, w, '%s %s %s' % (what, name, route))
                    else:
                        assert np.array_equal(arr, w), (what, name, route)
            if T >= 37 and not one_hot:
                assert want[0][0, 6] == -1 and want[0][0, 20] == -1 and want[0][-1, 0] == -1 and want[0][-1, T - 1] == -1
                assert not want[3][0, [1, 3, 6]].any() and want[3][0, 2] > 0 and not want[3][-1, 4] > 0


# ---- dir_diffusion_solve_local -------------------------------------------------------------------------------------------
LOCAL_T = [1, 63, 64, 65, SLAB - 1, SLAB, SLAB + 1, 600, 2048]      # chain, slab and limit edges


@pytest.fixture(scope='module')
def local_graphs():
    """{(T, k): (lidx [k,T] int32, lw [k,T] fp32)} from planted lists through dir_knn_graph: dead slots keep their raw ids
    (one of them 2^20 past the rows) with a weight of zero"""
    from dirtorch_amd import ops
    out = {}
    for T in LOCAL_T:
        for k in (1, 7, 50):
            if T < 10:
                idx, S = np.full((T, k), -1, np.int32), np.zeros((T, k), np.float32)
            else:
                idx, vals, _ = planted_lists(T, k, 3 * T + k)
                S = ops.knn_graph(_cuda(idx, np.int32), _cuda(vals), 3).cpu().numpy()
            out[T, k] = (np.ascontiguousarray(idx.T), np.ascontiguousarray(S.T))
    return out


def local_seeds(Q, T, seed):
    r = np.random.RandomState(seed)
    y = np.where(r.uniform(size=(Q, T)) < 0.15, r.uniform(0.1, 1.0, (Q, T)), 0).astype(np.float32)
    y[:, 0] = 0.5
    cid = np.arange(T, dtype=np.int32)[None, :].repeat(Q, axis=0)
    if T >= 63:
        cid[-1, 11] = -1
    return y, cid


def run_local(lidx, lw, y, cid, alpha, iters, pad):
    """f as an ndarray: through ops.diffusion_solve_local (pad = 0) or the raw ABI at ldt = T + pad, ldf = T + pad + 1"""
    from dirtorch_amd import _lib, ops
    Q, k, T = lidx.shape
    if pad == 0:
        f = ops.diffusion_solve_local(_cuda(lidx, np.int32), _cuda(lw), _cuda(y), None if cid is None else _cuda(cid, np.int32),
                                      alpha=alpha, iters=iters)
        assert f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (Q, T)
        return f.cpu().numpy()
    wf = torch.full((Q, T + pad + 1), 7.0, device='cuda')
    tabs = [_wide(lidx, pad, FAR), _wide(lw, pad, NAN), _wide(y, pad, NAN), _wide(cid, pad, -1)]
    _lib.call('dir_diffusion_solve_local', _lib.ptr(tabs[0]), _lib.ptr(tabs[1]), k, _lib.ptr(tabs[2]), _lib.ptr(tabs[3]), T + pad,
              Q, T, float(alpha), int(iters), _lib.ptr(wf), T + pad + 1, _lib.stream_ptr())
    got = wf.cpu().numpy()
    assert (got[:, T:] == 7.0).all(), 'the padding of f was written'
    return np.ascontiguousarray(got[:, :T])


@pytest.mark.parametrize('T', LOCAL_T)
def test_solve_local_bit_for_bit(local_graphs, T):
    """dir_diffusion_solve_local against solve_ref per query, bit for bit: k = 1, 7, 50, iters = 0, 1, 20, three queries
    with their own seeds on one graph, the last with a dead candidate (NaN); packed through ops and at a pitch through the
    ABI.  alpha = 0 gives y, a zero seed stays zero, and together or one at a time the queries give the same bits."""
    Q = 3
    for k in (1, 7, 50):
        lidx = np.ascontiguousarray(np.broadcast_to(local_graphs[T, k][0], (Q, k, T)))
        lw = np.ascontiguousarray(np.broadcast_to(local_graphs[T, k][1], (Q, k, T)))
        y, cid = local_seeds(Q, T, 7 * T + k)
        y[1] = 0
        for iters in (0, 1, 20):
            want = solve_local_ref(lidx, lw, y, cid, 0.99, iters)
            what = 'T %d k %d iters %d' % (T, k, iters)
            got = run_local(lidx, lw, y, cid, 0.99, iters, 0)
            assert_bits(got, want, what)
            assert_bits(run_local(lidx, lw, y, cid, 0.99, iters, 3), want, what + ' at a pitch')
            assert not np.nan_to_num(got[1]).any(), 'a zero seed stays zero'
            assert iters == 0 or got[0].any()
            assert T < 63 or (np.isnan(got[-1, 11]) and np.isnan(got).sum() == 1)
        assert_bits(run_local(lidx, lw, y, None, 0.0, 1, 0), y, 'alpha 0 returns y')
        alone = np.concatenate([run_local(lidx[q:q + 1], lw[q:q + 1], y[q:q + 1], cid[q:q + 1], 0.99, 20, 0) for q in range(Q)])
        assert_bits(alone, got, 'T %d k %d one query at a time' % (T, k))


@pytest.mark.parametrize('T', [65, SLAB + 1, 2048])
def test_solve_local_equals_the_full_solve_on_the_local_graph(local_graphs, T):
    """each query's result is ops.diffusion_solve's on that query's local graph as a one-column problem, bit for bit"""
    from dirtorch_amd import ops
    li, lv = local_graphs[T, 7]
    y, _ = local_seeds(2, T, T)
    got = run_local(np.stack([li, li]), np.stack([lv, lv]), y, None, 0.99, 20, 0)
    for q in range(2):
        full = ops.diffusion_solve(_cuda(li.T, np.int32), _cuda(lv.T), _cuda(y[q][:, None]), alpha=0.99, iters=20)
        assert_bits(got[q], full.cpu().numpy()[:, 0], 'T %d query %d' % (T, q))


def test_identity_candidates_equal_the_full_solve(planted):
    """identity candidates (T = N = 300) with y = Y[:, q]: the local graph is the graph and the result is column q of
    dir_diffusion_solve on all rows"""
    from dirtorch_amd import ops
    idx, S = planted
    N, k = idx.shape
    Q = 5
    gi, gs = _cuda(idx, np.int32), _cuda(S)
    r = np.random.RandomState(5)
    Y = np.where(r.uniform(size=(N, Q)) < 0.1, r.uniform(0.1, 1.0, (N, Q)), 0).astype(np.float32)
    cidx = torch.arange(N, dtype=torch.int32, device='cuda')[None, :].repeat(Q, 1)
    cid, lidx, lw, _ = ops.diffusion_subgraph(gi, gs, cidx, torch.ones(Q, N, device='cuda'), kq=0)
    assert torch.equal(cid, cidx) and torch.equal(lw, gs.t()[None].expand(Q, k, N))
    f = ops.diffusion_solve_local(lidx, lw, _cuda(np.ascontiguousarray(Y.T)), cid=cid, alpha=0.99, iters=20)
    F = ops.diffusion_solve(gi, gs, _cuda(Y), alpha=0.99, iters=20)
    assert_bits(f.cpu().numpy(), F.cpu().numpy().T, 'identity candidates')
    assert_bits(F.cpu().numpy(), solve_ref(idx, S, Y, 0.99, 20), 'and both are the restatement')


# ---- dir_diffusion_spread ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Q,N,T', [(1, 5, 3), (3, 300, 37), (70, 1000, 257)])
def test_spread_bit_for_bit(Q, N, T):
    """dir_diffusion_spread against spread_ref: an f below -2, a NaN f on a live candidate, dead slots with a finite f, ids
    past N among the dead; packed and at pitches of N + 3 / T + 2, the padding untouched"""
    from dirtorch_amd import _lib, ops
    r = np.random.RandomState(N)
    scores = r.uniform(-1, 1, (Q, N)).astype(np.float32)
    cid = np.stack([r.permutation(N)[:T] for _ in range(Q)]).astype(np.int32)
    f = r.uniform(-0.1, 1.0, (Q, T)).astype(np.float32)
    f[0, 0], f[-1, 1] = -2.5, np.nan
    cid[0, 2] = -1
    want = spread_ref(scores, cid, f)
    got = ops.diffusion_spread(_cuda(scores), _cuda(cid, np.int32), _cuda(f))
    assert_bits(got.cpu().numpy(), want, 'packed')
    assert want[0, cid[0, 0]] == -2 and want[-1, cid[-1, 1]] == -2 and (want.max(axis=1) <= 1).all()
    ws, wc, wf = _wide(scores, 3, 7.0), _wide(cid, 2, FAR), _wide(f, 2, NAN)
    _lib.call('dir_diffusion_spread', _lib.ptr(ws), N + 3, Q, N, _lib.ptr(wc), _lib.ptr(wf), T + 2, T, _lib.stream_ptr())
    raw = ws.cpu().numpy()
    assert (raw[:, N:] == 7.0).all(), 'the padding of the scores was written'
    assert_bits(raw[:, :N], want, 'at a pitch')
    view = _wide(scores, 3, 7.0)
    assert ops.diffusion_spread(view[:, :N], _cuda(cid, np.int32), _cuda(f)) .data_ptr() == view.data_ptr()
    assert_bits(view.cpu().numpy()[:, :N], want, 'a view, in place')


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rings():
    q, b, positives = two_rings()
    ring = np.zeros(len(b), np.int64)
    ring[positives[-1]] = 1
    return q, b, positives, ring, np.array([ring[p[0]] for p in positives])


def _own_ring_first(idx_row, val_row, ring, own, skip=0):
    """a ranked list: every candidate of the query's own ring before every candidate of the other ring, by score"""
    live = idx_row[skip:] >= 0
    mine = ring[idx_row[skip:][live]] == own
    v = val_row[skip:][live]
    return (not mine.any()) or (not (~mine).any()) or v[mine].min() > v[~mine].max()


@pytest.mark.parametrize('T,bound', [(128, 0.67), (256, 0.83)])
def test_diffuse_truncated_device_on_two_rings(rings, T, bound):
    """ranking.diffuse_truncated_device, k = 10, kq = 5, gamma = 3, alpha = 0.99, 20 iterations, restated from the device's own
    graph and lists: the ranked lists and the dense scores bit for bit; every own-ring candidate before every other-ring
    one for all 16 queries; the dense mAP above 0.67 (T = 128) / 0.83 (T = 256) where the cosine ranking has 0.564."""
    from dirtorch_amd import ranking
    q, b, positives, ring, qring = rings
    kw = dict(trunc=T, k=10, kq=5, gamma=3, alpha=0.99, iters=20)
    qd, bd = _cuda(q), _cuda(b)
    graph = ranking.knn_graph_device(bd, 10, gamma=3)
    idx, vals = ranking.diffuse_truncated_device(qd, bd, graph=graph, **kw)
    assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and tuple(idx.shape) == tuple(vals.shape) == (16, T)
    lists = tuple(t.cpu().numpy() for t in ranking.retrieve_device(qd, bd, T))
    cid, lidx, lw, y = subgraph_ref(graph[0].cpu().numpy(), graph[1].cpu().numpy(), lists[0], lists[1], 5, 3)
    f = solve_local_ref(lidx, lw, y, cid, 0.99, 20)
    _same((idx, vals), topk_ref_rows(f, T, ids=cid), 'ranked lists')
    _same(ranking.diffuse_truncated_device(q, b, **kw), (idx, vals), 'host arrays, the graph made inside')
    gi, gv = idx.cpu().numpy(), vals.cpu().numpy()
    for n in range(16):
        assert _own_ring_first(gi[n], gv[n], ring, qring[n]), n
    dense = ranking.diffuse_truncated_device(qd, bd, graph=graph, dense=True, **kw)
    assert tuple(dense.shape) == (16, 384) and dense.is_contiguous()
    base = ranking.similarity_device(qd, bd).cpu().numpy()
    assert_bits(dense.cpu().numpy(), spread_ref(base, cid, f), 'dense')
    got, cosine = mean_ap(dense.cpu().numpy(), positives), mean_ap(q @ b.T, positives)
    print('T %d: dense mAP %.4f (cosine %.4f)' % (T, got, cosine))
    assert cosine < 0.6 and got > bound


def test_diffuse_truncated_device_same_set(rings):
    """same_set=True on the database - the case diffuse_device refuses: the row itself is candidate 0 with a one-hot seed
    and ranks first, its own ring next; restated from the device's lists bit for bit"""
    from dirtorch_amd import ranking
    _, b, _, ring, _ = rings
    bd = _cuda(b)
    graph = ranking.knn_graph_device(bd, 10, gamma=3)
    kw = dict(trunc=64, k=10, kq=5, gamma=3, alpha=0.99, iters=20, graph=graph, same_set=True)
    idx, vals = ranking.diffuse_truncated_device(bd, bd, **kw)
    oi, ov = (t.cpu().numpy() for t in ranking.retrieve_device(bd, bd, 63, same_set=True))
    lists = (np.concatenate([np.arange(384, dtype=np.int32)[:, None], oi], axis=1), np.concatenate([np.ones((384, 1), np.float32), ov], axis=1))
    cid, lidx, lw, y = subgraph_ref(graph[0].cpu().numpy(), graph[1].cpu().numpy(), lists[0], lists[1], 5, 3, one_hot=True)
    f = solve_local_ref(lidx, lw, y, cid, 0.99, 20)
    _same((idx, vals), topk_ref_rows(f, 64, ids=cid), 'same_set')
    gi, gv = idx.cpu().numpy(), vals.cpu().numpy()
    assert np.array_equal(gi[:, 0], np.arange(384))
    for row in (0, 100, 200, 300):
        assert _own_ring_first(gi[row], gv[row], ring, ring[row], skip=1), row
    with pytest.raises(ValueError):
        ranking.diffuse_truncated_device(bd[:50], bd, **kw)
    with pytest.raises(ValueError, match='database'):
        ranking.diffuse_device(bd, bd, k=10, kq=5)       # the full solve still refuses it


def test_diffuse_truncated_device_through_an_index(rings):
    """graph lists and candidates from an IVFInt8Index over the same rows, every list probed, re-ranked in fp32: the
    dense mAP bound of T = 256 holds; an index of another size is refused"""
    from dirtorch_amd import ranking
    from dirtorch_amd.index import IVFInt8Index
    q, b, positives, _, _ = rings
    index = IVFInt8Index(b.shape[1], 4).train(b).add(b)
    kw = dict(trunc=256, k=10, kq=5, gamma=3, alpha=0.99, iters=20, index=index, nprobe=4)
    dense = ranking.diffuse_truncated_device(q, b, dense=True, rerank=384, **kw)
    assert mean_ap(dense.cpu().numpy(), positives) > 0.83
    idx, vals = ranking.diffuse_truncated_device(q, b, rerank=384, **kw)
    assert tuple(idx.shape) == (16, 256) and (idx >= 0).all() and not torch.isnan(vals).any()
    with pytest.raises(ValueError):
        ranking.diffuse_truncated_device(q, b[:300], **kw)


# ---- python -m dirtorch_amd.retrieve --diffusion 10 5 --diffusion-trunc 128 ----------------------------------------------------
def test_retrieve_cli_diffusion_trunc(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats): on a dataset with its own query list it writes
    the first --topk of diffuse_truncated_device's ranked lists; a dataset whose images are their own queries, which
    --diffusion alone refuses, is accepted and a row is left out of its own list"""
    import dir_oracle as O
    from dirtorch_amd import ranking
    N, Q, D, k = 200, 12, 32, 7
    x, qx = synth_descriptors(61, N, D), synth_descriptors(62, Q, D)
    np.save(str(tmp_path / 'feats.bdescs.npy'), x)
    np.save(str(tmp_path / 'feats.qdescs.npy'), qx)
    (tmp_path / 'db.txt').write_text(''.join('img%d.jpg c%d\n' % (i, i % 9) for i in range(N)))
    (tmp_path / 'q.txt').write_text(''.join('q%d.jpg c%d\n' % (i, i % 9) for i in range(Q)))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + key: v for key, v in sd.items()}}, str(tmp_path / 'ck.pt'))
    pkg = os.path.join(ROOT, 'deep-image-retrieval_amd')
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get('PYTHONPATH', ''))
    tail = ['--checkpoint', str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0', '--topk', str(k),
            '--diffusion', '10', '5']
    runs = {'own_queries': ['--dataset', 'ImageListLabelsQ("%s", "%s", root="%s")' % (tmp_path / 'db.txt', tmp_path / 'q.txt', tmp_path),
                            '--diffusion-trunc', '128'],
            'self_set': ['--dataset', 'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--diffusion-trunc', '64']}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve'] + flags + tail + ['--output', outs[name]], env=env)
             for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]

    def check(name, want):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), want, name)

    idx, vals = ranking.diffuse_truncated_device(qx, x, trunc=128, k=10, kq=5)
    check('own_queries', (idx[:, :k], vals[:, :k]))      # the first --topk of the ranked lists
    # a dataset whose queries are its rows is accepted with the flag: the row itself seeds the solve and is left out of its
    # list wherever it ranks (a hub among its neighbours can outscore it), the order of the others kept
    idx, vals = (t.cpu().numpy() for t in ranking.diffuse_truncated_device(x, x, trunc=64, k=10, kq=5, same_set=True))
    others = idx != np.arange(N)[:, None]
    assert (others.sum(axis=1) == 63).all() and (idx >= 0).all()
    check('self_set', (idx[others].reshape(N, 63)[:, :k], vals[others].reshape(N, 63)[:, :k]))

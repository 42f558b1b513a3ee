"""Truncated diffusion, the checks that need no GPU: the numpy restatement (tests/diffusion_trunc_ref.py) against the
properties the definition promises and on two_rings, the new symbols through header, ctypes table, ops and ranking, and
the argument errors of the three entry points (raised before anything is launched)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from diffusion_ref import dense_graph, exact_lists, knn_graph_ref, mean_ap, planted_lists, two_rings
from diffusion_trunc_ref import live_candidates, local_dense, solve_local_ref, spread_ref, subgraph_ref, truncated_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, KQ, GAMMA, ALPHA, ITERS = 10, 5, 3, 0.99, 20      # the two_rings setting


@pytest.fixture(scope='module')
def rings():
    q, b, positives = two_rings()
    idx, vals = exact_lists(b, b, K, True)
    S = knn_graph_ref(idx, vals, GAMMA)
    ring = np.zeros(len(b), np.int64)
    ring[positives[-1]] = 1                      # the last query lies on the second circle
    out = dict(q=q, b=b, positives=positives, idx=idx, S=S, ring=ring, qring=np.array([ring[p[0]] for p in positives]))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.fixture(scope='module')
def planted():
    idx, vals, _ = planted_lists(60, 7, 11)
    return idx, knn_graph_ref(idx, vals, GAMMA)


def test_identity_candidates_reproduce_the_graph(planted):
    idx, S = planted
    N, k = idx.shape
    cidx = np.tile(np.arange(N, dtype=np.int32), (2, 1))
    cvals = np.full((2, N), 0.5, np.float32)
    cid, lidx, lw, y = subgraph_ref(idx, S, cidx, cvals, 4, GAMMA)
    assert np.array_equal(cid, cidx)
    for q in range(2):
        assert np.array_equal(lw[q].T, S)
        assert np.array_equal(lidx[q].T, np.where(S != 0, idx, -1))
    assert np.array_equal(y[0, :4], np.full(4, 0.125, np.float32)) and not y[:, 4:].any()


def test_dead_candidates_are_rows_without_edges(planted):
    idx, S = planted
    N, k = idx.shape
    cidx = np.arange(20, 44, dtype=np.int32)[None, :].copy()
    cidx[0, 5], cidx[0, 9], cidx[0, 14] = -1, N + (1 << 20), cidx[0, 3]      # a hole, an id out of range, a later duplicate
    cvals = np.linspace(0.9, 0.2, 24, dtype=np.float32)[None, :]
    cid, lidx, lw, y = subgraph_ref(idx, S, cidx, cvals, 24, GAMMA)
    assert np.array_equal(live_candidates(cidx, N)[0], ~np.isin(np.arange(24), [5, 9, 14]))
    for a in (5, 9, 14):
        assert cid[0, a] == -1 and y[0, a] == 0
        assert (lidx[0][:, a] == -1).all() and not lw[0][:, a].any() and not np.signbit(lw[0][:, a]).any()
        assert not (lidx[0] == a).any(), 'no other row keeps an edge to a dead candidate'
    assert cid[0, 3] == cidx[0, 3] and (lidx[0] == 3).any(), 'the first slot of a duplicated id stays live'
    assert (lidx[0] >= 0).sum() > 24 and ((lidx[0] >= 0) == (lw[0] != 0)).all()
    # the rows that named the dropped ids (25, 29, 34 as global ids) lose exactly those edges
    full = subgraph_ref(idx, S, np.arange(20, 44, dtype=np.int32)[None, :], cvals, 24, GAMMA)
    kept = np.isin(full[1][0], [5, 9, 14], invert=True) & (full[1][0] >= 0)
    kept[:, [5, 9, 14]] = False
    assert np.array_equal(kept, lidx[0] >= 0)


@pytest.mark.parametrize('T', [1, 24, 60])
def test_the_local_matrix_is_symmetric_bit_for_bit(planted, T):
    idx, S = planted
    r = np.random.RandomState(T)
    cidx = np.stack([r.permutation(60)[:T] for _ in range(3)]).astype(np.int32)
    cid, lidx, lw, _ = subgraph_ref(idx, S, cidx, np.ones((3, T), np.float32), 0, GAMMA)
    full = dense_graph(idx, S)
    for q in range(3):
        A = local_dense(lidx[q], lw[q])
        assert np.array_equal(A, A.T)
        assert np.array_equal(A, full[np.ix_(cidx[q], cidx[q])]), 'a principal sub-matrix of S'
    assert T == 1 or lw.any()


def _own_ring_first(cid, f, ring, own, skip=0):
    """every candidate of the query's own ring scores above every candidate of the other ring"""
    live = cid[skip:] >= 0
    mine = ring[cid[skip:][live]] == own
    fl = f[skip:][live]
    return (not mine.any()) or (not (~mine).any()) or fl[mine].min() > fl[~mine].max()


@pytest.mark.parametrize('T,bound', [(128, 0.67), (256, 0.83)])
def test_two_rings_truncated(rings, T, bound):
    """k = 10, kq = 5, gamma = 3, alpha = 0.99, exact fp32 lists, 20 iterations: among the T candidates of each of the 16
    queries every own-ring row outranks every other-ring row, and the dense form has mAP > 0.67 (T = 128) / > 0.83
    (T = 256) where the cosine ranking has 0.564 (a numpy prototype measured 0.6755 and 0.8388)."""
    cid, f, dense = truncated_ref(rings['q'], rings['b'], (rings['idx'], rings['S']), T, KQ, GAMMA, ALPHA, ITERS)
    assert cid.shape == (16, T) and (cid >= 0).all() and not np.isnan(f).any()
    for q in range(16):
        assert _own_ring_first(cid[q], f[q], rings['ring'], rings['qring'][q]), q
    got = mean_ap(dense, rings['positives'])
    cosine = mean_ap(rings['q'] @ rings['b'].T, rings['positives'])
    print('T %d: dense mAP %.4f (cosine %.4f)' % (T, got, cosine))
    assert abs(cosine - 0.564) < 1e-3 and got > bound
    # the dense form: candidates above -2, everything else in [-5, -3] in cosine order
    inside = np.zeros(dense.shape, bool)
    np.put_along_axis(inside, cid.astype(np.int64), True, axis=1)
    assert (dense[inside] >= -2).all() and (dense[~inside] <= -3).all() and (dense[~inside] >= -5).all()


@pytest.mark.parametrize('T', [64, 128])
def test_self_mode_on_two_rings(rings, T):
    """database rows 0, 100, 200, 300 as their own queries, one-hot seed: the row itself ranks first, its own ring's
    candidates next"""
    b = rings['b']
    rows = np.array([0, 100, 200, 300])
    oi, ov = exact_lists(b, b, T - 1, True)
    lists = (np.concatenate([rows[:, None].astype(np.int32), oi[rows]], axis=1),
             np.concatenate([np.ones((4, 1), np.float32), ov[rows]], axis=1))
    cid, f, _ = truncated_ref(b[rows], b, (rings['idx'], rings['S']), T, KQ, GAMMA, ALPHA, ITERS, same_set=True, lists=lists)
    for n, row in enumerate(rows):
        assert cid[n, 0] == row and f[n].argmax() == 0 and f[n, 0] > f[n, 1:].max()
        assert _own_ring_first(cid[n], f[n], rings['ring'], rings['ring'][row], skip=1), row


def test_solve_local_ref_fixed_points(planted):
    idx, S = planted
    cidx = np.stack([np.arange(30), np.arange(30, 60)]).astype(np.int32)
    cidx[1, 7] = -1
    cid, lidx, lw, y = subgraph_ref(idx, S, cidx, np.full((2, 30), 0.7, np.float32), 5, GAMMA)
    got = solve_local_ref(lidx, lw, y, cid, 0.0, 1)
    assert np.isnan(got[1, 7]) and np.array_equal(np.delete(got, 7, axis=1), np.delete(y, 7, axis=1))
    assert not np.nan_to_num(solve_local_ref(lidx, lw, y, cid, ALPHA, 0)).any()
    assert not solve_local_ref(lidx, lw, np.zeros_like(y), None, ALPHA, 20).any()


def test_spread_ref_rules():
    scores = np.array([[0.5, -1.0, 1.0, 0.25, 0.0]], np.float32)
    cid = np.array([[3, -1, 0, 4]], np.int32)
    f = np.array([[0.75, 9.0, -2.5, np.nan]], np.float32)
    assert np.array_equal(spread_ref(scores, cid, f), np.array([[-2.0, -5.0, -3.0, 0.75, -2.0]], np.float32))


# ---- the interfaces ------------------------------------------------------------------------------------------------------
def _params(src, name):
    m = re.search(r'int %s\(([^)]*)\);' % name, src)
    assert m, 'include/dir_engine.h does not declare ' + name
    return [p.strip() for p in m.group(1).replace('\n', ' ').split(',')]


def test_header_ctypes_ops_and_ranking_agree_on_the_new_symbols():
    from dirtorch_amd import _lib, ops, ranking
    src = open(os.path.join(ROOT, 'include', 'dir_engine.h')).read()
    names = {
        'dir_diffusion_subgraph': ['idx', 'ldl', 'S', 'lds', 'N', 'k', 'cidx', 'cvals', 'ldc', 'Q', 'T', 'kq', 'gamma', 'one_hot',
                                   'cid', 'lidx', 'lw', 'y', 'ldt', 'stream'],
        'dir_diffusion_solve_local': ['lidx', 'lw', 'k', 'y', 'cid', 'ldt', 'Q', 'T', 'alpha', 'iters', 'f', 'ldf', 'stream'],
        'dir_diffusion_spread': ['scores', 'lds', 'Q', 'N', 'cid', 'f', 'ldt', 'T', 'stream'],
    }
    lib = _lib.load()
    for name, want_names in names.items():
        params = _params(src, name)
        assert [p.split()[-1].lstrip('*') for p in params] == want_names
        want = [ctypes.c_void_p if '*' in p else {'int': ctypes.c_int, 'float': ctypes.c_float}[p.split()[0]] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == want, name
        assert getattr(lib, name).argtypes == want
    assert 'int dir_diffusion_local_max_rows(void);' in src
    assert _lib.SIGNATURES['dir_diffusion_local_max_rows'] == (ctypes.c_int, [])
    assert lib.dir_diffusion_local_max_rows() == lib.dir_topk_max_k() == 2048 == ops.diffusion_local_max_rows()
    sig = inspect.signature(ops.diffusion_subgraph).parameters
    assert list(sig)[:7] == ['idx', 'S', 'cidx', 'cvals', 'kq', 'gamma', 'one_hot']
    assert sig['gamma'].default == 3 and sig['one_hot'].default is False
    sig = inspect.signature(ops.diffusion_solve_local).parameters
    assert list(sig) == ['lidx', 'lw', 'y', 'cid', 'alpha', 'iters']
    assert [sig[n].default for n in ('cid', 'alpha', 'iters')] == [None, 0.99, 20]
    assert list(inspect.signature(ops.diffusion_spread).parameters) == ['scores', 'cid', 'f']
    sig = inspect.signature(ranking.diffuse_truncated_device).parameters
    assert list(sig)[:13] == ['qdescs', 'bdescs', 'trunc', 'k', 'kq', 'gamma', 'alpha', 'iters', 'graph', 'index', 'same_set',
                              'dense', 'scratch_bytes']
    assert [sig[n].default for n in list(sig)[2:13]] == [1000, 50, 10, 3, 0.99, 20, None, None, False, False, 256 << 20]
    assert list(sig)[13] == 'search_kw'
    build = open(os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc', 'build.sh')).read()
    assert re.search(r'\bdiffusion_local\b', build)
    kernels = open(os.path.join(ROOT, 'deep-image-retrieval_amd', 'csrc', 'diffusion_local.hip')).read()
    assert 'fp contract(off)' in kernels and 'hipMalloc' not in kernels and 'atomicAdd' not in kernels


def test_cli_flag_is_declared_and_off_by_default():
    import argparse
    from dirtorch_amd import eval_dir
    parser = argparse.ArgumentParser()
    for names, kw in eval_dir.DIFFUSION_FLAGS:
        parser.add_argument(*names, **kw)
    assert eval_dir.diffusion_options(parser.parse_args([])) is None
    plain = eval_dir.diffusion_options(parser.parse_args(['--diffusion', '10', '5']))
    assert plain == dict(k=10, kq=5, alpha=0.99, gamma=3, iters=20), 'without the flag: the keywords of diffuse_device'
    got = eval_dir.diffusion_options(parser.parse_args(['--diffusion', '10', '5', '--diffusion-trunc', '128']))
    assert got == dict(plain, trunc=128)
    with pytest.raises(SystemExit):
        eval_dir.diffusion_options(parser.parse_args(['--diffusion-trunc', '128']))


def test_argument_errors_need_no_gpu():
    """Every DIR_ERR_INVALID case of the header for the three entries, with a non-null, 16-byte aligned host address for
    the pointers and a null stream: nothing is launched."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    raw = ctypes.create_string_buffer(4096 + 16)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) // 16 * 16)
    err = lib.dir_last_error
    big = lib.dir_topk_max_k() + 1
    nan = float('nan')

    def sub(idx=p, ldl=4, S=p, lds=4, N=9, k=4, cidx=p, cvals=p, ldc=6, Q=2, T=6, kq=3, gamma=3.0, one_hot=0, cid=p, lidx=p,
            lw=p, y=p, ldt=6):
        return lib.dir_diffusion_subgraph(idx, ldl, S, lds, N, k, cidx, cvals, ldc, Q, T, kq, gamma, one_hot, cid, lidx, lw, y,
                                          ldt, None)
    for name in ('N', 'k', 'Q', 'T', 'kq'):
        assert sub(**{name: -1}) == -1 and b'negative' in err(), name
    assert sub(ldl=3) == -1 and sub(lds=3) == -1 and b'ldl' in err()
    assert sub(ldc=5) == -1 and sub(ldt=5) == -1 and b'ldt' in err()
    assert sub(T=0) == -1 and sub(T=big, ldc=big, ldt=big) == -1 and b'dir_diffusion_local_max_rows' in err()
    assert sub(k=big, ldl=big, lds=big) == -1 and b'dir_topk_max_k' in err()
    assert sub(gamma=-1.0) == -1 and sub(gamma=nan) == -1 and b'gamma' in err()
    for name in ('idx', 'S', 'cidx', 'cvals', 'cid', 'lidx', 'lw', 'y'):
        assert sub(**{name: None}) == -1 and b'null' in err(), name
    assert sub(Q=1 << 22) == -1 and b'2^32' in err()      # a workgroup of 1024 threads per query
    assert sub(Q=0, idx=None, S=None, cidx=None, cvals=None, cid=None, lidx=None, lw=None, y=None) == 0

    def solve(lidx=p, lw=p, k=4, y=p, cid=p, ldt=6, Q=2, T=6, alpha=0.5, iters=2, f=p, ldf=6):
        return lib.dir_diffusion_solve_local(lidx, lw, k, y, cid, ldt, Q, T, alpha, iters, f, ldf, None)
    for name in ('k', 'Q', 'T', 'iters'):
        assert solve(**{name: -1}) == -1 and b'negative' in err(), name
    assert solve(ldt=5) == -1 and solve(ldf=5) == -1 and b'ldt' in err()
    assert solve(T=0) == -1 and solve(T=big, ldt=big, ldf=big) == -1 and b'dir_diffusion_local_max_rows' in err()
    assert solve(k=big) == -1 and b'dir_topk_max_k' in err()
    for alpha in (-0.1, 1.0, 1.5, nan):
        assert solve(alpha=alpha) == -1 and b'alpha' in err(), alpha
    for name in ('lidx', 'lw', 'y', 'f'):
        assert solve(**{name: None}) == -1 and b'null' in err(), name
    assert solve(Q=1 << 22) == -1 and b'2^32' in err()
    assert solve(Q=0, lidx=None, lw=None, y=None, cid=None, f=None) == 0

    def spread(scores=p, lds=9, Q=2, N=9, cid=p, f=p, ldt=6, T=6):
        return lib.dir_diffusion_spread(scores, lds, Q, N, cid, f, ldt, T, None)
    for name in ('Q', 'N', 'T'):
        assert spread(**{name: -1}) == -1 and b'negative' in err(), name
    assert spread(lds=8) == -1 and b'lds' in err()
    assert spread(ldt=5) == -1 and b'ldt' in err()
    assert spread(T=big, ldt=big) == -1 and b'dir_diffusion_local_max_rows' in err()
    for name in ('scores', 'cid', 'f'):
        assert spread(**{name: None}) == -1 and b'null' in err(), name
    assert spread(Q=1 << 16, N=1 << 16, lds=1 << 16) == -1 and b'Q * N' in err() and b'2^32' in err()
    assert spread(Q=1 << 21, N=1, lds=1, T=2048, ldt=2048) == -1 and b'Q * T' in err() and b'2^32' in err()
    assert spread(Q=0, scores=None, cid=None, f=None) == 0 and spread(N=0, lds=0, scores=None, cid=None, f=None) == 0


def test_python_argument_errors_need_no_gpu():
    import torch
    from dirtorch_amd import ops
    idx, S = torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 2)
    with pytest.raises(ValueError):
        ops.diffusion_subgraph(idx, S, idx, S)              # host tensors
    with pytest.raises(ValueError):
        ops.diffusion_solve_local(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, 3), torch.zeros(1, 3))
    with pytest.raises(ValueError):
        ops.diffusion_spread(torch.zeros(1, 5), torch.zeros(1, 3, dtype=torch.int32), torch.zeros(1, 3))

"""Diffusion re-ranking on the device (dir_knn_graph, dir_diffusion_seed, dir_diffusion_solve, ranking.knn_graph_device /
diffuse_device, the --diffusion flag of python -m dirtorch_amd.retrieve) against the numpy restatement of
tests/diffusion_ref.py.  The definition is a chain of single fp32 operations in a stated order, so with an integer gamma
everything is compared bit for bit; only powf (a non-integer gamma) has a bound."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diffusion_ref import (ISOLATED_ROW, SLAB, dense_graph, exact_lists, knn_graph_ref, mean_ap, planted_lists, seed_ref,
                           solve_ref, two_rings)
from index_util import cuda as _cuda, same as _same
from synth import synth_descriptors
from topk_ref import bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = 1 << 30      # an id in the padding of a list table: never to be read


def _wide(a, pad, fill):
    """a [rows, w] -> a CUDA buffer [rows, w + pad] holding it, `fill` in the padding"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    out = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out.cuda()


def assert_bits(got, want, what):
    assert got.shape == want.shape and not np.isnan(want).any(), what
    assert torch.equal(torch.from_numpy(bits(got).astype(np.int64)), torch.from_numpy(bits(want).astype(np.int64))), (
        what, np.argwhere(bits(got) != bits(want))[:5])


# ---- dir_knn_graph -----------------------------------------------------------------------------------------------------
def run_graph(idx, vals, gamma, pad):
    """S as an ndarray: through ops.knn_graph (pad = 0), or through the C ABI with list and graph pitches of k + pad - an id
    far outside the database and a NaN score in the lists' padding - whose own padding must come back untouched"""
    from dirtorch_amd import _lib, ops
    N, k = idx.shape
    if pad == 0:
        S = ops.knn_graph(_cuda(idx, np.int32), _cuda(vals), gamma)
        assert S.is_cuda and S.dtype == torch.float32 and tuple(S.shape) == (N, k) and S.is_contiguous()
        return S.cpu().numpy()
    wi, wv = _wide(idx, pad, FAR), _wide(vals, pad, float('nan'))
    ws = torch.full((N, k + pad), 7.0, dtype=torch.float32, device='cuda')
    _lib.call('dir_knn_graph', _lib.ptr(wi), _lib.ptr(wv), k + pad, N, k, float(gamma), _lib.ptr(ws), k + pad,
              _lib.stream_ptr())
    got = ws.cpu().numpy()
    assert (got[:, k:] == 7.0).all(), 'the padding of S was written'
    return np.ascontiguousarray(got[:, :k])


@pytest.mark.parametrize('N', [37, 300])
def test_knn_graph_bit_for_bit(N):
    """dir_knn_graph against knn_graph_ref, bit for bit: k = 1, 5, 10, 33 (an odd k leaves a one-sided last slot), gamma =
    0, 1, 3, contiguous and at a pitch of k + 3; a dead slot of every kind planted (the out-of-range id is 2^20 past the
    database: dereferencing it would fault), an isolated row, and the symmetry the definition promises."""
    for k in (1, 5, 10, 33):
        idx, vals, dead = planted_lists(N, k, 17 * N + k)
        for gamma in (0, 1, 3):
            want = knn_graph_ref(idx, vals, gamma)
            for pad in (0, 3):
                got = run_graph(idx, vals, gamma, pad)
                assert_bits(got, want, 'N %d k %d gamma %d pad %d' % (N, k, gamma, pad))
            for kind, (i, t) in dead.items():
                assert bits(got[i:i + 1, t:t + 1])[0, 0] == 0, kind      # +0
            assert not got[ISOLATED_ROW].any()
            A = dense_graph(idx, got)
            assert np.array_equal(A, A.T) and A.any()


def test_knn_graph_non_integer_gamma_within_powf():
    """gamma = 2.5 against the restatement in float64 at a relative 1e-5: powf is the one step that is not bit-defined
    (test_expand_lists_gpu.py has the precedent), and every number here is a weight that has also passed a sum of up to
    ten positive terms, a square root, a division and two products in fp32.  The zeros are where the restatement has
    them."""
    idx, vals, _ = planted_lists(300, 10, 5)
    want = knn_graph_ref(idx, vals, 2.5, dtype=np.float64)
    got = run_graph(idx, vals, 2.5, 0)
    assert np.array_equal(got == 0, want == 0)
    worst = np.abs(got - want)[want != 0] / want[want != 0]
    print('largest relative difference %.3g' % worst.max())
    assert worst.max() <= 1e-5


# ---- dir_diffusion_seed ------------------------------------------------------------------------------------------------
def seed_lists(Q, kq, N, seed):
    r = np.random.RandomState(seed)
    qidx = r.randint(0, N, (Q, kq)).astype(np.int32)
    qvals = r.uniform(0.1, 1.0, (Q, kq)).astype(np.float32)
    qidx[0, 3] = qidx[0, 1]                     # a duplicate id: the later slot wins
    qidx[0, 2], qvals[0, 2] = -1, np.nan        # dead slots: a hole,
    qidx[-1, 0] = N + (1 << 20)                 # an id out of range,
    qvals[-1, 1], qvals[-1, 4] = -0.25, 0.0     # a negative and a zero score
    return qidx, qvals


@pytest.mark.parametrize('Q', [1, 3, 70])
def test_diffusion_seed_bit_for_bit(Q):
    """dir_diffusion_seed against seed_ref, bit for bit, gamma 1 and 3, contiguous and at pitches of kq + 2 / Q + 3: a
    duplicate id whose later slot wins, a hole, an id out of range, a negative and a zero score; the zero fill included."""
    from dirtorch_amd import _lib, ops
    N, kq = 37, 5
    qidx, qvals = seed_lists(Q, kq, N, 40 + Q)
    for gamma in (1, 3):
        want = seed_ref(qidx, qvals, N, gamma)
        Y = ops.diffusion_seed(_cuda(qidx, np.int32), _cuda(qvals), N, gamma)
        assert Y.is_cuda and Y.dtype == torch.float32 and tuple(Y.shape) == (N, Q) and Y.is_contiguous()
        assert_bits(Y.cpu().numpy(), want, 'Q %d gamma %d' % (Q, gamma))
        wi, wv = _wide(qidx, 2, FAR), _wide(qvals, 2, float('nan'))
        wy = torch.full((N, Q + 3), 7.0, dtype=torch.float32, device='cuda')
        _lib.call('dir_diffusion_seed', _lib.ptr(wi), _lib.ptr(wv), kq + 2, Q, kq, N, float(gamma), _lib.ptr(wy), Q + 3,
                  _lib.stream_ptr())
        got = wy.cpu().numpy()
        assert (got[:, Q:] == 7.0).all(), 'the padding of Y was written'
        assert_bits(np.ascontiguousarray(got[:, :Q]), want, 'Q %d gamma %d at a pitch' % (Q, gamma))


# ---- dir_diffusion_solve -----------------------------------------------------------------------------------------------
def run_solve(idx, S, Y, alpha, iters, pad):
    """F as an ndarray: through ops.diffusion_solve (pad = 0), or through the C ABI with every pitch = width + pad (an id
    far outside the database / NaN in the padding of the operands) and a workspace of exactly the size asked for, filled
    with NaN; the padding of F must come back untouched"""
    from dirtorch_amd import _lib, ops
    (N, k), Q = idx.shape, Y.shape[1]
    if pad == 0:
        F = ops.diffusion_solve(_cuda(idx, np.int32), _cuda(S), _cuda(Y), alpha=alpha, iters=iters)
        assert F.is_cuda and F.dtype == torch.float32 and tuple(F.shape) == (N, Q) and F.is_contiguous()
        return F.cpu().numpy()
    wi, ws, wy = _wide(idx, pad, FAR), _wide(S, pad, float('nan')), _wide(Y, pad, float('nan'))
    wf = torch.full((N, Q + pad), 7.0, dtype=torch.float32, device='cuda')
    need = ctypes.c_size_t(0)
    _lib.call('dir_diffusion_workspace_bytes', N, Q, ctypes.byref(need))
    work = torch.full((need.value // 4,), float('nan'), dtype=torch.float32, device='cuda')
    _lib.call('dir_diffusion_solve', _lib.ptr(wi), k + pad, _lib.ptr(ws), k + pad, N, k, _lib.ptr(wy), Q + pad, Q, float(alpha),
              int(iters), _lib.ptr(wf), Q + pad, _lib.ptr(work), need.value, _lib.stream_ptr())
    got = wf.cpu().numpy()
    assert (got[:, Q:] == 7.0).all(), 'the padding of F was written'
    return np.ascontiguousarray(got[:, :Q])


def solve_graph(N, k, seed):
    """a planted graph: dead slots, ids out of range and all"""
    idx, vals, _ = planted_lists(N, k, seed)
    return idx, knn_graph_ref(idx, vals, 3)


def solve_seeds(N, Q, seed):
    """sparse non-negative seed columns, column 1 zero between non-zero ones"""
    r = np.random.RandomState(seed)
    Y = np.where(r.uniform(size=(N, Q)) < 0.15, r.uniform(0.1, 1.0, (N, Q)), 0).astype(np.float32)
    if Q >= 3:
        Y[:, 1] = 0
    return Y


SOLVE_N = [37, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 3]
SOLVE_Q = [1, 3, 4, 5, 64, 70]
SOLVE_SETTINGS = [(1, 0, 0.5), (10, 1, 0.0), (33, 3, 0.99), (10, 20, 0.99)]      # (k, iters, alpha): every value of each


@pytest.mark.parametrize('N', SOLVE_N)
def test_diffusion_solve_bit_for_bit(N):
    """dir_diffusion_solve against solve_ref, bit for bit.  N: below, just below, at and just past one slab of the dot
    products (ops.diffusion_slab_rows()) and past two; Q = 1, 3, 4, 5, 64, 70: non-multiples of four, one column group,
    more column groups than half a workgroup; (k, iters, alpha) = (1, 0, 0.5), (10, 1, 0), (33, 3, 0.99), (10, 20, 0.99) at
    every (N, Q); each case contiguous and through the raw ABI at pitches of width + 3.  Column 1 is zero between
    non-zero ones and must stay zero."""
    from dirtorch_amd import ops
    assert ops.diffusion_slab_rows() == SLAB
    for k, iters, alpha in SOLVE_SETTINGS:
        idx, S = solve_graph(N, k, 10 * N + k)
        for Q in SOLVE_Q:
            Y = solve_seeds(N, Q, 100 * N + Q)
            want = solve_ref(idx, S, Y, alpha, iters)
            what = 'N %d Q %d k %d iters %d alpha %g' % (N, Q, k, iters, alpha)
            for pad in (0, 3):
                got = run_solve(idx, S, Y, alpha, iters, pad)
                assert_bits(got, want, '%s pad %d' % (what, pad))
            if Q >= 3:
                assert not got[:, 1].any() and (iters == 0 or got[:, 0].any()), what


def test_diffusion_solve_fixed_points_and_repeatability():
    """alpha = 0 gives F = Y after one iteration and iters = 0 gives zeros, bit for bit; the same call twice gives the same
    bits; and the columns solved in one call of Q or in two calls of Q / 2 give the same bits (Q = 4, 64, 70)."""
    N = 2 * SLAB + 3
    for Q in (4, 64, 70):
        (idx, S), Y = solve_graph(N, 10, 77), solve_seeds(N, Q, 78 + Q)
        assert_bits(run_solve(idx, S, Y, 0.0, 1, 0), Y, 'alpha 0')
        assert not run_solve(idx, S, Y, 0.99, 0, 0).any()
        one = run_solve(idx, S, Y, 0.99, 20, 0)
        assert_bits(run_solve(idx, S, Y, 0.99, 20, 0), one, 'the same call twice')
        h = Q // 2
        two = np.concatenate([run_solve(idx, S, np.ascontiguousarray(Y[:, :h]), 0.99, 20, 0),
                              run_solve(idx, S, np.ascontiguousarray(Y[:, h:]), 0.99, 20, 0)], axis=1)
        assert_bits(two, one, 'Q %d as two calls' % Q)


# ---- end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rings():
    q, b, positives = two_rings()
    idx, vals = exact_lists(b, b, 10, True)
    S = knn_graph_ref(idx, vals, 3)
    qidx, qvals = exact_lists(q, b, 5, False)
    Y = seed_ref(qidx, qvals, len(b), 3)
    F64 = np.linalg.solve(np.eye(len(b)) - 0.99 * dense_graph(idx, S).astype(np.float64), Y.astype(np.float64))
    return q, b, positives, F64


def test_diffuse_device_on_two_rings(rings):
    """ranking.diffuse_device with exact lists, k = 10, kq = 5, gamma = 3, alpha = 0.99, 50 iterations: mAP 1.0 where the
    cosine ranking has 0.564, and the top 10 of the dense fp64 solve for all 16 queries; with the graph made beforehand
    (knn_graph_device) the same bits; a query set that is the database raises ValueError."""
    from dirtorch_amd import ranking
    q, b, positives, F64 = rings
    kw = dict(k=10, kq=5, gamma=3, alpha=0.99, iters=50)
    qd, bd = _cuda(q), _cuda(b)
    scores = ranking.diffuse_device(qd, bd, **kw)
    assert scores.is_cuda and scores.dtype == torch.float32 and tuple(scores.shape) == (16, 384) and scores.is_contiguous()
    got = scores.cpu().numpy()
    assert mean_ap(got, positives) == 1.0 and mean_ap(q @ b.T, positives) < 0.6
    for c in range(16):
        assert np.array_equal(np.argsort(-got[c], kind='stable')[:10], np.argsort(-F64[:, c], kind='stable')[:10]), c
    graph = ranking.knn_graph_device(bd, 10, gamma=3)
    assert graph[0].dtype == torch.int32 and tuple(graph[1].shape) == (384, 10)
    assert torch.equal(ranking.diffuse_device(qd, bd, graph=graph, **kw), scores)
    assert torch.equal(ranking.diffuse_device(q, b, **kw), scores)      # host arrays are uploaded
    with pytest.raises(ValueError, match='database'):
        ranking.diffuse_device(bd, bd, **kw)
    with pytest.raises(ValueError, match='database'):
        ranking.diffuse_device(b, b, **kw)
    with pytest.raises(TypeError):
        ranking.diffuse_device(qd, bd, nprobe=2, **kw)       # search keywords without an index


def test_diffuse_device_through_an_index(rings):
    """The graph's lists and the queries' from an Int8Index over the same rows, re-ranked at 4 k: mAP 1.0; an index of
    another size is refused."""
    from dirtorch_amd import ranking
    from dirtorch_amd.index import Int8Index
    q, b, positives, _ = rings
    index = Int8Index(b.shape[1]).add(b)
    got = ranking.diffuse_device(q, b, k=10, kq=5, gamma=3, alpha=0.99, iters=50, index=index, rerank=40)
    assert mean_ap(got.cpu().numpy(), positives) == 1.0
    with pytest.raises(ValueError):
        ranking.diffuse_device(q, b[:300], k=10, kq=5, index=index)


# ---- python -m dirtorch_amd.retrieve --diffusion ---------------------------------------------------------------------------
def test_retrieve_cli_diffusion(tmp_path):
    """The CLI in fresh processes on synthetic descriptors (--load-feats) of a dataset with its own query list:
    --diffusion 10 5 writes ops.topk over diffuse_device's scores; the same invocation without the flag writes what it
    writes today, retrieve_device's lists."""
    import dir_oracle as O
    from dirtorch_amd import ops, ranking
    N, Q, D, k = 120, 12, 32, 7
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
    base = ['--dataset', 'ImageListLabelsQ("%s", "%s", root="%s")' % (tmp_path / 'db.txt', tmp_path / 'q.txt', tmp_path),
            '--checkpoint', str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0', '--topk', str(k)]
    runs = {'diffusion': ['--diffusion', '10', '5'], 'plain': []}
    outs = {name: str(tmp_path / (name + '.npz')) for name in runs}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve'] + base + ['--output', outs[name]] + flags,
                              env=env) for name, flags in runs.items()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]

    def check(name, want):
        npz = np.load(outs[name])
        assert sorted(npz.files) == ['idx', 'scores'] and npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
        _same((npz['idx'], npz['scores']), want, name)

    check('diffusion', ops.topk(ranking.diffuse_device(qx, x, k=10, kq=5), k))
    check('plain', ranking.retrieve_device(qx, x, k))

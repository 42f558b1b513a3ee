"""Top-k retrieval on the device (dir_topk, ops.topk, ranking.retrieve_device, python -m dirtorch_amd.retrieve) against
the numpy restatement of tests/topk_ref.py.  No tolerance anywhere: indices are compared with ==, scores bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from topk_ref import bits, topk_ref_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE = 16384          # csrc/topk.hip kTopkSlice (test_slice_constant pins it through the workspace size)


def _cuda(a, dtype=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _max_k():
    from dirtorch_amd import ops
    return ops.topk_max_k()


def _run(scores, k, ids=None, exclude=None, lds=None):
    """(idx, vals) ndarrays of ops.topk on host arrays; lds > N puts the rows (and the id table) into wider buffers."""
    from dirtorch_amd import ops
    scores = np.asarray(scores, np.float32)
    Q, N = scores.shape
    dev_ids = None
    if lds is None:
        dev = _cuda(scores, np.float32)
        if ids is not None:
            dev_ids = _cuda(ids)
    else:
        wide = torch.full((Q, lds), float('nan'), dtype=torch.float32, device='cuda')   # the padding must not be read
        wide[:, :N] = _cuda(scores, np.float32)
        dev = wide[:, :N]
        if ids is not None:
            wide_ids = torch.full((Q, lds), 2 ** 30, dtype=torch.int32, device='cuda')
            wide_ids[:, :N] = _cuda(ids)
            dev_ids = wide_ids[:, :N]
    idx, vals = ops.topk(dev, k, exclude=None if exclude is None else _cuda(exclude), ids=dev_ids)
    assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda and vals.is_cuda
    assert tuple(idx.shape) == (Q, k) and tuple(vals.shape) == (Q, k)
    return idx.cpu().numpy(), vals.cpu().numpy()


def _same(got, want, what=''):
    assert (got[0] == want[0]).all(), (what, np.argwhere(got[0] != want[0])[:5], got[0].ravel()[:8], want[0].ravel()[:8])
    assert (bits(got[1]) == bits(want[1])).all(), (what, np.argwhere(bits(got[1]) != bits(want[1]))[:5])


def _check(scores, k, ids=None, exclude=None, lds=None, want=None):
    got = _run(scores, k, ids, exclude, lds)
    _same(got, want if want is not None else topk_ref_rows(scores, k, ids, exclude), 'k = %d' % k)
    return got


def _boundary_rows():
    r = np.random.RandomState(61)
    N, Q = SLICE + 37, 5
    scores = r.standard_normal((Q, N)).astype(np.float32)
    scores[1] = np.round(scores[1] * 8) / 8                     # a row with ties
    scores[2, SLICE + 5] = 10                                   # the best item in the ragged last slice
    scores[3, N - 1] = 11                                       # ... in the last column
    scores[4, SLICE - 1], scores[4, SLICE] = 9, 9               # a tie across the slice boundary, both best
    return scores


def _ks():
    return (1, 37, 100, _max_k())


def test_slice_constant():
    from dirtorch_amd import _lib
    import ctypes
    need = ctypes.c_size_t(1)
    _lib.call('dir_topk_workspace_bytes', 1, SLICE, 1, ctypes.byref(need))
    assert need.value == 0
    _lib.call('dir_topk_workspace_bytes', 1, SLICE + 1, 1, ctypes.byref(need))
    assert need.value > 0


def test_slice_boundary_ragged_tail_and_row_pitch():
    scores = _boundary_rows()
    N = scores.shape[1]
    for k in _ks():
        idx, _ = _check(scores, k, lds=N + 11)
        assert idx[2, 0] == SLICE + 5 and idx[3, 0] == N - 1 and idx[4, 0] == SLICE
        if k > 1:
            assert idx[4, 1] == SLICE - 1


def test_k_larger_than_a_slices_share():
    r = np.random.RandomState(62)
    N, k = 3 * SLICE + 5, _max_k()
    scores = r.standard_normal((3, N)).astype(np.float32)
    scores[:, SLICE + 100:SLICE + 100 + k] += 100               # the whole list lies in the second slice
    scores[2] = np.round(scores[2] * 4) / 4
    idx, _ = _check(scores, k)
    assert (idx >= SLICE + 100).all() and (idx < SLICE + 100 + k).all()


@pytest.mark.parametrize('N', [1, 2, 5, 64, 65])
def test_tiny_rows(N):
    r = np.random.RandomState(63 + N)
    scores = np.round(r.standard_normal((4, N)) * 2).astype(np.float32) / 2
    for k in sorted({1, N}):
        _check(scores, k)


def _three_levels(Q, N, seed, ones=None):
    r = np.random.RandomState(seed)
    scores = r.randint(-1, 2, (Q, N)).astype(np.float32)        # {-1, 0, 1}: everything ties
    if ones is not None:                                        # a row with few ones: the cut falls among the zeros
        scores[0] = np.where(r.rand(N) < ones, 1, np.where(r.rand(N) < 0.5, 0, -1))
    minus = scores.copy()
    zeros = np.flatnonzero(scores.ravel() == 0)
    minus.ravel()[zeros[::3]] = -0.0
    assert np.signbit(minus).sum() > (scores < 0).sum()
    return scores, minus


@pytest.mark.parametrize('N', [3000, 2 * SLICE + 9])
def test_ties_across_the_cut_and_signed_zeros(N):
    scores, minus = _three_levels(3, N, 64, ones=0.003)
    scores[2] = 0.25                                            # an all-equal row
    minus[2] = 0.25
    n_one = (scores == 1).sum(axis=1)
    n_top = ((scores == 1) | (scores == 0)).sum(axis=1)
    for k in (n_one[1] // 2, n_one[0] + 500, n_one[1] + 300):
        k = int(min(k, _max_k()))
        # the cut of row 0 or 1 is inside a tie group (that spans the slices when there are several)
        assert (n_one[1] > k) or (n_one[0] < k < n_top[0]) or (n_one[1] < k < n_top[1])
        plus = _check(scores, k)
        got = _check(minus, k)
        assert (plus[0] == got[0]).all() and (plus[1] == got[1]).all()      # same lists; -0.0 == 0.0 by value
        assert (got[0][2] == N - 1 - np.arange(k)).all()        # all equal: the k largest indices, descending


def test_non_finite_scores():
    r = np.random.RandomState(65)
    N = SLICE + 700
    scores = r.standard_normal((6, N)).astype(np.float32)
    scores[0, [5, SLICE + 9]] = np.inf
    scores[0, [7, N - 1]] = -np.inf
    scores[1, r.choice(N, 9, replace=False)] = np.nan           # a few NaNs: they never make a list of numbers
    scores[2] = np.nan                                          # only NaNs: the largest indices
    scores[3] = np.nan                                          # fewer than k numbers: the NaNs fill the tail by descending index
    numbers = r.choice(N, 40, replace=False)
    scores[3, numbers] = r.standard_normal(40).astype(np.float32)
    scores[3, numbers[0]] = -np.inf
    scores[4] = -np.inf
    scores[4, 3] = np.nan                                       # -inf ranks before NaN
    scores[5] = np.nan
    scores[5, N - 1] = np.array([0x7fc01234], np.uint32).view(np.float32)[0]    # a payload comes back as stored
    for k in (1, 37, 100):
        idx, vals = _check(scores, k)
        assert np.isfinite(vals[1]).all() and bits(vals[5, :1])[0] == 0x7fc01234
        assert (idx[2] == N - 1 - np.arange(k)).all() and np.isnan(vals[2]).all()
        if k > 40:
            assert idx[3, 39] == numbers[0] and np.isnan(vals[3, 40:]).all() and (np.diff(idx[3, 40:]) < 0).all()
    idx, vals = _check(scores[4:5, :200], 200)
    assert idx[0, -1] == 3 and np.isnan(vals[0, -1]) and np.isinf(vals[0, :-1]).all()


def test_exclude():
    scores = _boundary_rows()
    N = scores.shape[1]
    best = int(np.argmax(scores[0]))
    # the best item; the last column; the first column past a slice boundary; the last column where it is the best; nobody
    exclude = np.array([best, N - 1, SLICE, N - 1, -1], np.int32)
    for k in (1, 100):
        idx, _ = _check(scores, k, exclude=exclude, lds=N + 5)
        assert (idx[:4] != exclude[:4, None]).all()
    first = _run(scores, 1)[0][:, 0]
    assert first[0] == best and first[3] == N - 1
    small = scores[:, :100].copy()
    idx, vals = _check(small, 100, exclude=np.array([17, 99, 0, 5, -1], np.int32))
    assert (idx[:4, -1] == -1).all() and np.isnan(vals[:4, -1]).all() and idx[4, -1] >= 0


def test_ids_permuted_with_holes_and_ties_broken_by_id():
    r = np.random.RandomState(66)
    N, Q = SLICE + 37, 3
    scores = np.round(r.standard_normal((Q, N)) * 4).astype(np.float32) / 4      # heavy ties
    ids = np.stack([r.permutation(5 * N)[:N] for _ in range(Q)]).astype(np.int32)
    ids[r.rand(Q, N) < 0.05] = -1
    ids[0, int(np.argmax(scores[0]))] = -1                      # the best column is a hole
    exclude = np.array([-1, ids[1, 3], ids[2, N - 1]], np.int32)
    for k in (1, 37, _max_k()):
        _check(scores, k, ids=ids)
        _check(scores, k, ids=ids, exclude=exclude, lds=N + 3)
    flat = np.zeros((1, 300), np.float32)
    tid = r.permutation(300).astype(np.int32)[None]
    idx, _ = _check(flat, 300, ids=tid)
    assert (idx[0] == 299 - np.arange(300)).all()                # by id, whatever the column
    few = tid.copy()
    few[0, 10:] = -1
    idx, vals = _check(flat, 300, ids=few)
    assert (idx[0, 10:] == -1).all() and np.isnan(vals[0, 10:]).all()


def test_merging_block_lists_equals_the_whole_row():
    from dirtorch_amd import ops
    scores = _boundary_rows()
    N = scores.shape[1]
    dev = _cuda(scores, np.float32)
    for k in _ks():
        ci, cv = [], []
        for b0 in range(0, N, 7001):
            i, v = ops.topk(dev[:, b0:b0 + 7001], k)
            ci.append(torch.where(i >= 0, i + b0, i))
            cv.append(v)
        idx, vals = ops.topk(torch.cat(cv, dim=1), k, ids=torch.cat(ci, dim=1))
        whole = ops.topk(dev, k)
        assert torch.equal(idx, whole[0]) and torch.equal(vals.view(torch.int32), whole[1].view(torch.int32))
        _same((idx.cpu().numpy(), vals.cpu().numpy()), topk_ref_rows(scores, k), 'merged, k = %d' % k)


def test_rank_counts_at_the_returned_indices_are_the_positions():
    from dirtorch_amd import ops
    r = np.random.RandomState(67)
    N, Q, k = 2 * SLICE + 100, 6, 300
    scores = _cuda(np.round(r.standard_normal((Q, N)) * 16) / 16, np.float32)
    idx, vals = ops.topk(scores, k)
    counts, pscores = ops.rank_counts(scores, idx)
    assert (counts.cpu().numpy() == np.arange(k)[None]).all()
    assert torch.equal(pscores.view(torch.int32), vals.view(torch.int32))
    again = ops.topk(scores, k)
    assert torch.equal(idx, again[0]) and torch.equal(vals.view(torch.int32), again[1].view(torch.int32))


def test_argument_checks():
    from dirtorch_amd import ops
    scores = torch.zeros(3, 50, device='cuda')
    for bad_k in (0, 51, _max_k() + 1):
        with pytest.raises(ValueError):
            ops.topk(scores, bad_k)
    with pytest.raises(TypeError):
        ops.topk(scores.double(), 1)
    with pytest.raises(TypeError):
        ops.topk(scores, 1, exclude=torch.zeros(3, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError):
        ops.topk(scores, 1, ids=torch.zeros(3, 49, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        ops.topk(scores.cpu(), 1)
    idx, vals = ops.topk(scores[:0], 5)
    assert tuple(idx.shape) == (0, 5) and tuple(vals.shape) == (0, 5)
    idx, _ = ops.topk(torch.zeros(50, 3, device='cuda').t(), 2)     # a view that is not row-major: copied, not misread
    assert idx.cpu().tolist() == [[49, 48]] * 3


# ---- ranking.retrieve_device -------------------------------------------------------------------------------------------
def test_retrieve_device_on_exact_planes():
    """tests/exact_planes.py operands: every score is one fp32 number under any chunking, so the lists of every setting
    equal the restatement's on the fp64 reference."""
    import exact_planes as E
    from dirtorch_amd import ranking
    Q, N, D = 97, 32768 + 255, 512
    q, d = E.operands('pair-1', Q, N, D, 'cuda', 7)
    want_scores = E.reference(q, d).cpu().numpy()
    for k in (1, 100):
        want = topk_ref_rows(want_scores, k)
        settings = {'default': {}, 'three query chunks': dict(scratch_bytes=4 * N * 40), 'database blocks': dict(db_rows=7001),
                    'both': dict(scratch_bytes=4 * 7001 * 33, db_rows=7001)}
        for name, kw in settings.items():
            idx, vals = ranking.retrieve_device(q, d, k, **kw)
            assert idx.dtype == torch.int32 and vals.dtype == torch.float32 and idx.is_cuda
            _same((idx.cpu().numpy(), vals.cpu().numpy()), want, '%s, k = %d' % (name, k))


def test_retrieve_device_same_set():
    """A square case on small integers (every product and sum exact in fp32, and nearly every score tied)."""
    from dirtorch_amd import ranking
    r = np.random.RandomState(68)
    N, D = 600, 64
    x = r.randint(-3, 4, (N, D)).astype(np.float32)
    scores = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    own = np.arange(N, dtype=np.int32)
    for k in (1, 20, N):
        want = topk_ref_rows(scores, k, exclude=own)
        for kw in ({}, dict(scratch_bytes=4 * N * 250), dict(db_rows=177), dict(db_rows=177, scratch_bytes=4 * 177 * 250)):
            if k > kw.get('db_rows', N):
                continue                                         # (a block offers at least k rows: same call as without)
            idx, vals = ranking.retrieve_device(x, x, k, same_set=True, **kw)
            _same((idx.cpu().numpy(), vals.cpu().numpy()), want, '%r, k = %d' % (kw, k))
            assert (idx.cpu().numpy() != own[:, None]).all()
    idx, vals = ranking.retrieve_device(x, x, N, same_set=True)
    assert (idx[:, -1] == -1).all() and torch.isnan(vals[:, -1]).all()
    _same(tuple(t.cpu().numpy() for t in ranking.retrieve_device(x[:50], x, 20)), topk_ref_rows(scores[:50], 20))
    with pytest.raises(ValueError):
        ranking.retrieve_device(x[:50], x, 20, same_set=True)
    with pytest.raises(ValueError):
        ranking.retrieve_device(x, x, N + 1)


# ---- python -m dirtorch_amd.retrieve ----------------------------------------------------------------------------------
def test_retrieve_cli_text_and_npz(tmp_path):
    """The CLI in fresh processes, --load-feats on synthetic descriptors with a synthetic checkpoint: the text output parses
    back to the .npz output, both equal retrieve_device, and a same-set dataset never lists a query as its own neighbour."""
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
    outs = {'txt': str(tmp_path / 'out' / 'pairs.txt'), 'npz': str(tmp_path / 'pairs.npz')}
    procs = [subprocess.Popen([sys.executable, '-m', 'dirtorch_amd.retrieve', '--dataset',
                               'ImageListLabels("%s", root="%s")' % (tmp_path / 'db.txt', tmp_path), '--checkpoint',
                               str(tmp_path / 'ck.pt'), '--whiten', '', '--load-feats', str(tmp_path), '--gpu', '0',
                               '--topk', str(k), '--output', out], env=env) for out in outs.values()]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    idx, vals = (t.cpu().numpy() for t in ranking.retrieve_device(x, x, k, same_set=True))
    npz = np.load(outs['npz'])
    assert sorted(npz.files) == ['idx', 'scores']
    _same((npz['idx'], npz['scores']), (idx, vals), 'npz')
    assert npz['idx'].dtype == np.int32 and npz['scores'].dtype == np.float32
    lines = open(outs['txt']).read().splitlines()
    assert lines[0] == '# query_image, map_image, score' and len(lines) == 1 + N * k
    rows = [l.split(', ') for l in lines[1:]]
    assert [row[0] for row in rows] == ['img%d.jpg' % (i // k) for i in range(N * k)]
    assert all(row[0] != row[1] for row in rows)
    txt_idx = np.array([int(row[1][3:-4]) for row in rows], np.int32).reshape(N, k)
    txt_vals = np.array([float(row[2]) for row in rows], np.float64).astype(np.float32).reshape(N, k)
    _same((txt_idx, txt_vals), (idx, vals), 'text')

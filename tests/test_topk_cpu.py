"""Top-k retrieval, host side (no GPU): the numpy restatement the GPU tests compare against (tests/topk_ref.py) is pinned to
the stable argsort it restates and to the count dir_rank_counts defines, and the library's argument checks - which run
before anything is launched - are exercised through the C ABI."""
import ctypes

import numpy as np

from topk_ref import bits, topk_ref


def _tie_heavy_rows():
    """NaN-free fp32 rows over 2, 3, 7 and 10^5 score levels, some zeros written as -0.0."""
    r = np.random.RandomState(51)
    for levels in (2, 3, 7, 10 ** 5):
        for N in (1, 2, 257, 1500, 2003):
            s = (r.randint(0, levels, N) - levels // 2).astype(np.float32) / np.float32(levels)
            zeros = np.flatnonzero(s == 0)
            s[zeros[::2]] = -0.0
            yield s


def test_restatement_is_the_reversed_stable_argsort_on_nan_free_rows():
    n = 0
    for s in _tie_heavy_rows():
        N = len(s)
        want = np.argsort(s, kind='stable')[::-1]
        for k in sorted({1, min(N, 10), N}):
            idx, vals = topk_ref(s, k)
            assert idx.dtype == np.int32 and vals.dtype == np.float32
            assert (idx == want[:k]).all(), (N, k)
            assert (bits(vals) == bits(s[want[:k]])).all(), (N, k)     # stored bits: a -0.0 stays -0.0
        n += 1
    assert n == 20


def test_position_of_a_number_is_its_rank_count():
    """dir_rank_counts: counts[p] = #{j : s_j > s_p, or s_j == s_p and j > p}, NaN items ranking before nothing."""
    r = np.random.RandomState(52)
    for levels in (2, 3, 7, 10 ** 5):
        for nan_rate in (0.0, 0.05):
            N = 400
            s = (r.randint(0, levels, N) - levels // 2).astype(np.float32)
            s[r.rand(N) < 0.1] = -0.0
            s[r.rand(N) < nan_rate] = np.nan
            idx, _ = topk_ref(s, N)
            pos = np.empty(N, np.int64)
            pos[idx] = np.arange(N)
            j = np.arange(N)
            for p in np.flatnonzero(~np.isnan(s)):
                with np.errstate(invalid='ignore'):
                    before = (s > s[p]) | ((s == s[p]) & (j > p))
                assert pos[p] == before.sum(), (levels, p)


def test_nans_come_last_by_descending_id():
    s = np.array([np.nan, -np.inf, 1.0, np.nan, np.inf, -0.0, 0.0, np.nan], np.float32)
    idx, vals = topk_ref(s, 8)
    assert idx.tolist() == [4, 2, 6, 5, 1, 7, 3, 0]
    assert (bits(vals) == bits(s[idx])).all()
    ids = np.array([10, 3, 7, 40, 2, 9, 8, 20])
    idx, _ = topk_ref(s, 8, ids=ids)
    assert idx.tolist() == [2, 7, 9, 8, 3, 40, 20, 10]            # zeros tie: id 9 before id 8; NaNs 40, 20, 10
    idx, vals = topk_ref(np.full(5, np.nan, np.float32), 3)
    assert idx.tolist() == [4, 3, 2] and np.isnan(vals).all()


def test_short_rows_end_in_filler():
    s = np.array([0.5, 0.25, 0.75], np.float32)
    idx, vals = topk_ref(s, 3, exclude=2)
    assert idx.tolist() == [0, 1, -1] and vals[:2].tolist() == [0.5, 0.25] and bits(vals)[2] == bits(np.float32(np.nan))
    idx, vals = topk_ref(s, 3, ids=np.array([-1, 5, -1]))
    assert idx.tolist() == [5, -1, -1] and vals[0] == 0.25 and np.isnan(vals[1:]).all()
    idx, vals = topk_ref(s, 2, ids=np.array([4, 5, 6]), exclude=6)
    assert idx.tolist() == [4, 5]
    idx, _ = topk_ref(s, 3, exclude=-1)
    assert idx.tolist() == [2, 0, 1]


def test_merging_block_lists_through_ids_is_the_whole_row_list():
    r = np.random.RandomState(53)
    for levels in (3, 10 ** 5):
        N = 5003
        s = (r.randint(0, levels, N) - levels // 2).astype(np.float32)
        s[r.rand(N) < 0.01] = np.nan
        for k in (1, 37, 700):
            for block in (701, 2500):
                ci, cv = [], []
                for b0 in range(0, N, block):
                    i, v = topk_ref(s[b0:b0 + block], min(k, len(s[b0:b0 + block])))
                    ci.append(np.where(i >= 0, i + b0, -1))
                    cv.append(v)
                idx, vals = topk_ref(np.concatenate(cv), k, ids=np.concatenate(ci))
                want_i, want_v = topk_ref(s, k)
                assert (idx == want_i).all() and (bits(vals) == bits(want_v)).all(), (levels, k, block)


# ---- the library's host-side checks ------------------------------------------------------------------------------------
def _workspace(lib, Q, N, k):
    need = ctypes.c_size_t(12345)
    assert lib.dir_topk_workspace_bytes(Q, N, k, ctypes.byref(need)) == 0, (Q, N, k)
    return need.value


def test_max_k_and_workspace_bytes():
    from dirtorch_amd import _lib
    lib = _lib.load()
    assert lib.dir_topk_max_k() >= 1024
    kmax = lib.dir_topk_max_k()
    sizes = [1, 1000, 16384, 16385, 40000, 1006322, 2 ** 31 - 1]
    for Q in (1, 70):
        for k in (1, 100, kmax):
            w = [_workspace(lib, Q, N, k) for N in sizes if N >= k]
            assert w == sorted(w) and w[-1] > 0, (Q, k, w)
    for N in (40000, 1006322):
        w = [_workspace(lib, 70, N, k) for k in (1, 10, 100, 1024, kmax)]
        assert w == sorted(w) and w[0] > 0
        w = [_workspace(lib, Q, N, 100) for Q in (1, 2, 70, 20000, 70000, 200000)]
        assert w == sorted(w)
    need = ctypes.c_size_t(0)
    for Q, N, k in ((1, 100, 0), (1, 100, 101), (1, 10 ** 6, kmax + 1), (-1, 100, 1)):
        assert lib.dir_topk_workspace_bytes(Q, N, k, ctypes.byref(need)) == -1
    assert lib.dir_topk_workspace_bytes(1, 100, 1, None) == -1


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    kmax = lib.dir_topk_max_k()
    Q, N = 2, 40000
    scores = (ctypes.c_float * 16)()
    idx = (ctypes.c_int * 16)()
    vals = (ctypes.c_float * 16)()
    ws = (ctypes.c_char * 16)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    need = _workspace(lib, Q, N, 10)
    assert need > 0

    def run(k=10, lds=N, n=N, scores_=p(scores), idx_=p(idx), vals_=p(vals), ws_=p(ws), ws_bytes=need, q=Q):
        return lib.dir_topk(scores_, lds, q, n, k, None, None, idx_, vals_, ws_, ws_bytes, None)

    assert run(k=0) == -1 and b'k < 1' in lib.dir_last_error()
    assert run(k=-3) == -1
    assert run(k=N + 1, n=N) == -1
    assert run(k=101, n=100, lds=100) == -1 and b'exceeds' in lib.dir_last_error()
    assert run(k=kmax + 1) == -1 and b'exceeds' in lib.dir_last_error()
    assert run(lds=N - 1) == -1 and b'lds' in lib.dir_last_error()
    assert run(idx_=None) == -1 and b'null' in lib.dir_last_error()
    assert run(vals_=None) == -1 and run(scores_=None) == -1
    assert run(ws_bytes=need - 1) == -1 and b'workspace' in lib.dir_last_error()
    assert run(ws_=None) == -1 and b'workspace' in lib.dir_last_error()
    assert run(q=-1) == -1
    assert run(q=0) == 0                                # no query: DIR_OK, nothing launched

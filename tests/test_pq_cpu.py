"""The product-quantised index, host side (no GPU): the library exports the new entry points and checks their arguments
before anything is launched, and the numpy restatement (tests/pq_ref.py) gives the hand-computed codes, tables and scores
of small cases - the tie rule and a NaN row among them."""
import ctypes

import numpy as np
import pytest

import pq_ref
from topk_ref import bits


def test_library_exports_the_pq_entry_points():
    from dirtorch_amd import _lib, ops
    lib = _lib.load()
    for name, nargs in (('dir_pq_max_m', 0), ('dir_pq_encode', 9), ('dir_pq_lut', 8), ('dir_pq_scan', 9)):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES, 'no ctypes signature for ' + name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.dir_pq_max_m() == 128 == ops.pq_max_m()       # one query's table, M KiB, fits the 160 KiB of LDS


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 512)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)           # the scan wants its tables 16-byte aligned
    err = lib.dir_last_error

    def encode(X=p, ldx=64, N=5, D=64, M=8, cb=p, codes=p, ldc=8):
        return lib.dir_pq_encode(X, ldx, N, D, M, cb, codes, ldc, None)

    def lut(q=p, ldq=64, Q=3, D=64, M=8, cb=p, out=p):
        return lib.dir_pq_lut(q, ldq, Q, D, M, cb, out, None)

    def scan(lut=p, Q=3, M=8, codes=p, ldc=8, N=40, scores=p, lds=40):
        return lib.dir_pq_scan(lut, Q, M, codes, ldc, N, scores, lds, None)

    assert encode(N=-1) == -1 and b'negative' in err()
    assert lut(Q=-1) == -1 and b'negative' in err()
    assert scan(Q=-1) == -1 and scan(N=-1, lds=0) == -1 and b'negative' in err()
    for f in (encode, lut):
        assert f(D=0) == -1 and b'D < 1' in err()
        assert f(D=131080) == -1 and b'exceeds' in err()                 # above dir_index_i8_max_dim()
        assert f(M=0) == -1 and f(M=129, D=129 * 2) == -1 and b'dir_pq_max_m' in err()
        assert f(M=7) == -1 and b'divide' in err()                       # 64 % 7 != 0
    assert scan(M=0) == -1 and scan(M=129, ldc=132) == -1 and b'dir_pq_max_m' in err()
    assert encode(ldx=63) == -1 and b'ldx' in err()
    assert lut(ldq=63) == -1 and b'ldq' in err()
    assert encode(ldc=4) == -1 and encode(ldc=10) == -1 and b'ldc' in err()      # below M; no multiple of 4
    assert scan(ldc=4) == -1 and scan(ldc=10) == -1 and b'ldc' in err()
    assert scan(lds=39) == -1 and b'lds' in err()
    for name in ('X', 'cb', 'codes'):
        assert encode(**{name: None}) == -1 and b'null' in err(), name
    for name in ('q', 'cb', 'out'):
        assert lut(**{name: None}) == -1 and b'null' in err(), name
    for name in ('lut', 'codes', 'scores'):
        assert scan(**{name: None}) == -1 and b'null' in err(), name
    off = ctypes.c_void_p(p.value + 2)
    assert scan(lut=off) == -1 and scan(codes=off) == -1 and b'aligned' in err()
    assert encode(N=0) == 0 and lut(Q=0) == 0 and scan(Q=0) == 0 and scan(N=0, lds=0) == 0       # DIR_OK, nothing launched
    assert encode(N=0, X=None, codes=None) == 0


# ---- the restatement on hand-computed cases ----------------------------------------------------------------------------
def _codebooks(M, dsub, fill=100.0):
    """every centroid far away (`fill` in every column): a case places the few it needs"""
    return np.full((M, 256, dsub), fill, np.float32)


def test_restatement_encoding_by_hand():
    """D = 4, M = 2.  Sub-space 0: centroid 3 = (1, 2), centroid 200 = (1, 3); sub-space 1: centroids 7 and 9 both (0, 0) -
    a tie, the smaller index wins - and centroid 255 = (5, 5)."""
    cb = _codebooks(2, 2)
    cb[0, 3], cb[0, 200] = (1, 2), (1, 3)
    cb[1, 7], cb[1, 9], cb[1, 255] = (0, 0), (0, 0), (5, 5)
    x = np.array([[1, 2.4, 0.5, 0.5],       # (1, 2) is 0.16 away, (1, 3) 0.36; (0, 0) 0.5, (5, 5) 40.5
                  [1, 2.6, 4, 4],           # (1, 3); (5, 5)
                  [1, 2.5, 2.5, 2.5],       # 0.25 from both (exact in fp32): centroid 3; 12.5 from both: centroid 7
                  [0, 0, 0, 0]], np.float32)
    assert pq_ref.encode(x, cb).tolist() == [[3, 7], [200, 255], [3, 7], [3, 7]]
    d = pq_ref.distances(x, cb, 0)
    assert d.dtype == np.float32 and d.shape == (4, 256)
    assert bits(d[0, 3]) == bits(np.float32(0) + (np.float32(2.4) - np.float32(2)) * (np.float32(2.4) - np.float32(2)))
    assert d[2, 3] == 0.25 and d[2, 200] == 0.25 and d[3, 3] == 5.0
    # the chain runs over the columns in order, every step rounded: 4097^2 = 16785409 rounds to ...408, and each + 1 after
    # it is a tie that falls back to ...408; the correctly rounded sum is ...412
    cb3 = _codebooks(1, 3, 0.0)
    v = np.array([[4097.0, 1.0, 1.0]], np.float32)
    want = (np.float32(0) + np.float32(4097) * np.float32(4097) + np.float32(1)) + np.float32(1)
    assert bits(pq_ref.distances(v, cb3, 0)[0, 0]) == bits(want)
    assert want != np.float32(np.float64(4097) ** 2 + 2)                                    # not the correctly rounded sum


def test_restatement_nan_rows_and_nan_centroids():
    """A NaN in a row: code 0 in the sub-space it falls into, the other sub-space as usual.  A NaN centroid is never chosen
    over a number, not even as centroid 0; all-NaN distances give code 0."""
    cb = _codebooks(2, 2)
    cb[0, 5], cb[1, 6] = (1, 1), (2, 2)
    x = np.array([[np.nan, 1, 2, 2], [1, 1, 2, np.nan], [1, 1, 2, 2]], np.float32)
    assert pq_ref.encode(x, cb).tolist() == [[0, 6], [5, 0], [5, 6]]
    cb[0, 0] = np.nan
    cb[0, 5] = np.nan
    assert pq_ref.encode(x[2:], cb).tolist() == [[1, 6]]            # 0 and 5 are NaN: the first of the equal others
    cb[0] = np.nan
    assert pq_ref.encode(x[2:], cb).tolist() == [[0, 6]]
    inf = np.array([[np.inf, 0, 2, 2]], np.float32)                 # every distance +inf: the smallest index
    assert pq_ref.encode(inf, _codebooks(2, 2)).tolist() == [[0, 0]]


def test_restatement_tables_and_scores_by_hand():
    cb = _codebooks(2, 2, 0.0)
    cb[0, 1], cb[0, 2] = (1, 0), (0.5, -2)
    cb[1, 0], cb[1, 255] = (3, 3), (-1, 4)
    q = np.array([[2, 1, 1, -1], [0, 0, 0, 0]], np.float32)
    t = pq_ref.lut(q, cb)
    assert t.dtype == np.float32 and t.shape == (2, 2, 256)
    assert t[0, 0, 1] == 2 and t[0, 0, 2] == -1 and t[0, 1, 0] == 0 and t[0, 1, 255] == -5 and t[0, 0, 7] == 0
    assert not t[1].any() and not np.signbit(t[1]).any()            # +0 + 0 * c: +0
    codes = np.array([[1, 255], [2, 0], [7, 7]], np.uint8)
    s = pq_ref.scan(t, codes)
    assert s.dtype == np.float32 and s.tolist() == [[-3, -1, 0], [0, 0, 0]]
    # the chain runs m = 0, 1, 2: (2^24 + 1) + 1 stays 2^24 twice, 1 + 1 + 2^24 would not
    t3 = np.zeros((1, 3, 256), np.float32)
    t3[0, 0, 0], t3[0, 1, 0], t3[0, 2, 0] = 2.0 ** 24, 1, 1
    assert pq_ref.scan(t3, np.zeros((1, 3), np.uint8))[0, 0] == 2.0 ** 24
    t3[0, 0, 0], t3[0, 2, 0] = 1, 2.0 ** 24
    assert pq_ref.scan(t3, np.zeros((1, 3), np.uint8))[0, 0] == 2.0 ** 24 + 2
    # -0.0 entries: +0 + -0 = +0; inf - inf: NaN
    t3[0, :, 0] = -0.0
    assert bits(pq_ref.scan(t3, np.zeros((1, 3), np.uint8)))[0, 0] == 0
    t3[0, :, 0] = (np.inf, -np.inf, 1)
    assert np.isnan(pq_ref.scan(t3, np.zeros((1, 3), np.uint8))[0, 0])


def test_restatement_search_and_reconstruction_error():
    r = np.random.RandomState(7)
    D, M = 12, 3
    cb = r.standard_normal((M, 256, D // M)).astype(np.float32)
    x = r.standard_normal((50, D)).astype(np.float32)
    q = r.standard_normal((4, D)).astype(np.float32)
    codes = pq_ref.encode(x, cb)
    for n in range(0, 50, 7):                                        # a plain loop, one row and one sub-space at a time
        for m in range(M):
            d = [np.float32(0)] * 256
            for j in range(256):
                for c in range(4):
                    t = x[n, 4 * m + c] - cb[m, j, c]
                    d[j] = d[j] + t * t
            assert codes[n, m] == int(np.argmin(np.array(d)))        # (argmin: the first of equal minima)
    idx, vals = pq_ref.search_ref(q, x, cb, 5)
    s = pq_ref.scan(pq_ref.lut(q, cb), codes)
    for i in range(4):
        order = np.argsort(s[i], kind='stable')[::-1][:5]
        assert (idx[i] == order).all() and (bits(vals[i]) == bits(s[i][order])).all()
    own = np.array([3, 10, 20, 49], np.int32)
    idx2, _ = pq_ref.search_ref(q, x, cb, 5, exclude=own)
    assert (idx2 != own[:, None]).all()
    recon = np.concatenate([cb[m, codes[:, m]] for m in range(M)], axis=1).astype(np.float64)
    assert pq_ref.reconstruction_error(x, cb, codes) == pytest.approx(((x - recon) ** 2).sum() / 50, rel=1e-12)

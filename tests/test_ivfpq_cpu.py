"""The IVF-PQ index, host side (no GPU): the library exports the new entry points and checks their arguments before anything
is launched, the wrappers and the class refuse what they can refuse without a device, the numpy restatement
(tests/ivfpq_ref.py) gives the hand-computed residual, coarse term and score of a small case, and the property behind the
feature holds on the data the GPU tests use: residual codes reconstruct better than flat ones."""
import ctypes

import numpy as np
import pytest

import index_ref
import ivf_ref
import ivfpq_ref
import pq_ref
from synth import synth_descriptors
from topk_ref import bits


def test_library_exports_the_ivfpq_entry_points():
    from dirtorch_amd import _lib, ops
    lib = _lib.load()
    for name, nargs in (('dir_ivfpq_scan_cols', 0), ('dir_ivfpq_base', 12), ('dir_ivfpq_scan', 18)):
        assert hasattr(lib, name), 'missing export ' + name
        assert name in _lib.SIGNATURES, 'no ctypes signature for ' + name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
    assert lib.dir_ivfpq_scan_cols() == 1024 == ops.ivfpq_scan_cols()


def test_argument_errors_need_no_gpu():
    """DIR_ERR_INVALID (-1) before anything is launched: the pointers below are host memory no kernel may touch."""
    from dirtorch_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 512)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 63) // 64 * 64)           # the scan wants its tables 16-byte aligned
    err = lib.dir_last_error

    def base(q=p, ldq=64, Q=3, c=p, ldc=64, nlist=4, D=64, M=8, probe=p, nprobe=2, out=p):
        return lib.dir_ivfpq_base(q, ldq, Q, c, ldc, nlist, D, M, probe, nprobe, out, None)

    def scan(lut=p, base=p, Q=3, M=8, codes=p, ldc=8, ids=p, N=40, list_off=p, nlist=4, probe=p, col_off=p, nprobe=2,
             scores=p, out_ids=p, lds=64, width=50):
        return lib.dir_ivfpq_scan(lut, base, Q, M, codes, ldc, ids, N, list_off, nlist, probe, col_off, nprobe, scores,
                                  out_ids, lds, width, None)

    for name in ('Q', 'nlist', 'nprobe'):
        assert base(**{name: -1}) == -1 and b'negative' in err(), name
    assert base(D=0) == -1 and b'D < 1' in err()
    assert base(D=131080, ldq=131080, ldc=131080) == -1 and b'exceeds' in err()
    assert base(M=0) == -1 and base(M=129, D=258, ldq=258, ldc=258) == -1 and b'dir_pq_max_m' in err()
    assert base(M=7) == -1 and b'divide' in err()
    assert base(ldq=63) == -1 and base(ldc=63) == -1 and b'ld' in err()
    for name in ('q', 'c', 'probe', 'out'):
        assert base(**{name: None}) == -1 and b'null' in err(), name
    assert base(Q=0) == 0 and base(nprobe=0) == 0 and base(Q=0, q=None, out=None) == 0

    for name in ('Q', 'N', 'nlist', 'nprobe', 'width'):
        assert scan(**{name: -1}) == -1 and b'negative' in err(), name
    assert scan(M=0) == -1 and scan(M=129, ldc=132) == -1 and b'dir_pq_max_m' in err()
    assert scan(ldc=4) == -1 and scan(ldc=10) == -1 and b'ldc' in err()          # below M; no multiple of 4
    assert scan(lds=49) == -1 and b'lds' in err()
    for name in ('lut', 'base', 'codes', 'ids', 'list_off', 'probe', 'col_off', 'scores', 'out_ids'):
        assert scan(**{name: None}) == -1 and b'null' in err(), name
    off = ctypes.c_void_p(p.value + 2)
    assert scan(lut=off) == -1 and scan(codes=off) == -1 and b'aligned' in err()
    assert scan(Q=0) == 0 and scan(width=0, lds=0) == 0                           # nothing to do: DIR_OK, nothing launched


def test_wrappers_and_class_refuse_host_tensors_and_bad_shapes():
    """What ops.ivfpq_base / ops.ivfpq_scan and retrieve's flags refuse before they touch a device."""
    import torch
    from dirtorch_amd import ops, retrieve
    f, i, u = torch.zeros(3, 64), torch.zeros(3, 2, dtype=torch.int32), torch.zeros(40, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match='device'):
        ops.ivfpq_base(f, torch.zeros(4, 64), i, 8)
    with pytest.raises(ValueError, match='device'):
        ops.ivfpq_scan(torch.zeros(3, 8, 256), torch.zeros(3, 2), u, torch.zeros(40, dtype=torch.int32),
                       torch.zeros(5, dtype=torch.int32), i, i)
    base = ['--dataset', 'X', '--checkpoint', 'none', '--output', 'o.npz', '--index', 'ivfpq']
    with pytest.raises(SystemExit, match='nlist'):
        retrieve.main(base + ['--pq-m', '8'])
    with pytest.raises(SystemExit, match='pq-m'):
        retrieve.main(base + ['--nlist', '4'])


# ---- the restatement on a hand-computed case ---------------------------------------------------------------------------
def test_restatement_by_hand():
    """D = 4, M = 2, two lists.  A residual, a coarse term and a score written out literally."""
    centroids = np.array([[1, 0, 0, 0], [0.5, 0.25, -1, 2]], np.float32)
    x = np.array([[1.5, 0.25, 0, -1], [0.1, 0.25, 3, 2]], np.float32)
    r = ivfpq_ref.residuals(x, centroids, [0, 1])
    assert r.dtype == np.float32 and r[0].tolist() == [0.5, 0.25, 0, -1]
    assert bits(r[1, 0]) == bits(np.float32(0.1) - np.float32(0.5)) and r[1, 1:].tolist() == [0, 4, 0]
    q = np.array([[2, 4, 1, -1], [0, 0, 0, 0]], np.float32)
    b = ivfpq_ref.base(q, centroids, 2)
    assert b.dtype == np.float32 and b.shape == (2, 2)
    # list 1: s_0 = (0 + 2 * 0.5) + 4 * 0.25 = 2, s_1 = (0 + 1 * -1) + -1 * 2 = -3, base = (0 + 2) + -3 = -1
    assert b[0].tolist() == [2, -1] and not bits(b[1]).any()                 # a zero query: +0 (the chains start at +0)
    bp = ivfpq_ref.base(q, centroids, 2, probe=np.array([[1, -1, 1], [0, 1, -1]], np.int32))
    assert bp[0, 0] == -1 and np.isnan(bp[0, 1]) and bp[0, 2] == -1 and bp[1, 0] == 0 and np.isnan(bp[1, 2])
    # the order: sub-space sums first, then their sum.  (2^24 + 1) + 1 column by column would stay 2^24; s_0 = 2^24 and
    # s_1 = 1 + 1 = 2 give 2^24 + 2
    big = ivfpq_ref.base(np.array([[2.0 ** 24, 0, 1, 1]], np.float32), np.ones((1, 4), np.float32), 2)
    assert big[0, 0] == 2.0 ** 24 + 2
    assert ivfpq_ref.base(np.array([[2.0 ** 24, 1, 1, 0]], np.float32), np.ones((1, 4), np.float32), 1)[0, 0] == 2.0 ** 24
    # a score: the chain starts at the coarse term
    cb = np.zeros((2, 256, 2), np.float32)
    cb[0, 5], cb[1, 9] = (0.5, 0.25), (0, -1)
    assert pq_ref.encode(r[:1], cb).tolist() == [[5, 9]]                     # the residual IS those centroids
    t = pq_ref.lut(q, cb)
    assert t[0, 0, 5] == 2 and t[0, 1, 9] == 1
    s = ivfpq_ref.scan(t, b[:, [0]], np.array([[5, 9]], np.uint8))
    assert s.dtype == np.float32 and s[0, 0] == (np.float32(2) + np.float32(2)) + np.float32(1) == 5     # = <q, x_0> exactly
    start = np.array([[2.0 ** 24], [-0.0]], np.float32)
    t[0, 0, 5], t[0, 1, 9] = 1, 1
    t[1] = -0.0
    s = ivfpq_ref.scan(t, start, np.array([[5, 9]], np.uint8))
    assert s[0, 0] == 2.0 ** 24 and bits(s[1, 0]) == 0x80000000              # -0 + -0 + -0 stays -0: the padding's identity


def test_restatement_store_and_search_agree_with_a_plain_loop():
    """build / search against a loop over the lists: ids ascend inside a list, the codes are those of the residuals to the
    row's own centroid, and a query's lists are the top-k of base + table entries over the rows of its probed lists."""
    r = np.random.RandomState(160)
    D, nlist, M, k = 12, 4, 3, 9
    x, q = synth_descriptors(8, 70, D), synth_descriptors(9, 6, D)
    centroids = synth_descriptors(10, nlist, D)
    cb = (r.standard_normal((M, 256, D // M)) * 0.3).astype(np.float32)
    store = ivfpq_ref.build(x, centroids, cb)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    assert (store['lists'] == lists).all() and store['list_off'][-1] == 70 and store['codes'].shape == (70, M)
    for l in range(nlist):
        members = store['ids'][store['list_off'][l]:store['list_off'][l + 1]]
        assert (np.diff(members) > 0).all() and (lists[members] == l).all()
        want = pq_ref.encode(x[members] - centroids[l][None, :], cb)
        assert (store['codes'][store['list_off'][l]:store['list_off'][l + 1]] == want).all()
    t = pq_ref.lut(q, cb)
    b = ivfpq_ref.base(q, centroids, M)
    own = r.randint(0, 70, 6).astype(np.int32)
    from topk_ref import topk_ref_rows
    for nprobe in (1, 2, nlist):
        probed = ivf_ref.probe(*index_ref.quantize(q), centroids, nprobe)
        for exclude in (None, own):
            got = ivfpq_ref.search(q, x, centroids, cb, k, nprobe, exclude=exclude)
            for i in range(6):
                ids, scores = [], []
                for l in probed[i]:
                    for n in range(store['list_off'][l], store['list_off'][l + 1]):
                        acc = b[i, l]
                        for m in range(M):
                            acc = acc + t[i, m, store['codes'][n, m]]
                        ids.append(store['ids'][n])
                        scores.append(acc)
                want = topk_ref_rows(np.array([scores], np.float32), k, ids=np.array([ids], np.int32),
                                     exclude=None if exclude is None else exclude[i:i + 1])
                assert (got[0][i] == want[0][0]).all() and (bits(got[1][i]) == bits(want[1][0])).all(), (nprobe, i)


# ---- the property behind the feature -----------------------------------------------------------------------------------
def test_residual_codes_reconstruct_better_than_flat_codes():
    """synth_descriptors(6, 3000, 64), M = 8, nlist = 16, ten Lloyd iterations each, seed 0, codebooks trained in numpy: the
    mean squared reconstruction error of the residual codes is below that of flat PQ codes (0.1402 against 0.1761, a ratio
    of 0.80, when this was written); and with nprobe = 1 no query of synth_descriptors(5, 33, 64) has fewer than 100
    candidates (tests/test_ivfpq_gpu.py relies on it at k = 100)."""
    x = synth_descriptors(6, 3000, 64)
    centroids, cb_res = ivfpq_ref.train(x, 16, 8, iters=10, seed=0)
    cb_flat = ivfpq_ref.train_codebooks(x, 8, iters=10, seed=0)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    res = ivfpq_ref.residuals(x, centroids, lists)
    err_res = pq_ref.reconstruction_error(res, cb_res, pq_ref.encode(res, cb_res))
    err_flat = pq_ref.reconstruction_error(x, cb_flat, pq_ref.encode(x, cb_flat))
    print('reconstruction error %.4f residual, %.4f flat: ratio %.3f' % (err_res, err_flat, err_res / err_flat))
    assert np.isfinite([err_res, err_flat]).all() and err_res < err_flat
    lens = np.bincount(lists, minlength=16)
    q = synth_descriptors(5, 33, 64)
    cand = lens[ivf_ref.probe(*index_ref.quantize(q), centroids, 1)[:, 0]]
    print('list sizes %d .. %d, smallest candidate set %d' % (lens.min(), lens.max(), cand.min()))
    assert cand.min() >= 100

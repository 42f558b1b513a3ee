"""numpy restatement of the binary descriptor index (include/dir_engine.h: dir_quantize_rows_bin, dir_similarity_bin), for
the binary-index tests.  The definition is a fixed chain of single fp32 operations and an exact integer sum, so the device
results are compared bit for bit:

    bit k = sign bit of x_k clear (k < D; -0.0 codes as 0), bit k & 7 of byte k >> 3, zero past D
    sumabs, sumsq: 64 chains, chain l over k = 256 j + 4 l + e (j ascending, e = 0 .. 3), then l += l ^ d for d = 32 .. 1
    scale = sumsq / sumabs;  an inf / NaN row: zero bits, scale NaN;  sumabs zero or a sum infinite: zero bits, scale +0
    score[q][n] = ((float)t * sq[q]) * sb[n],  t = sum_{k < D} qc[q][k] * (+1 where bit k of row n is set, else -1)
"""
import numpy as np

from index_ref import quantize as quantize_i8
from synth import synth_descriptors
from topk_ref import topk_ref_rows

MAX_DIM = 131072                                    # 127 * 131072 < 2^24 <= 127 * 132105


def width(D):
    """bytes of a stored row of bits: D rounded up to 128, divided by 8"""
    return (D + 127) // 128 * 16


def _row_sums(v):
    """v [N, D] float32, non-negative -> the sum of every row in the definition's order, float32 [N]"""
    N, D = v.shape
    J = (D + 255) // 256
    pad = np.zeros((N, J * 256), np.float32)
    pad[:, :D] = v
    pad = pad.reshape(N, J, 64, 4)
    s = np.zeros((N, 64), np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        for j in range(J):
            for e in range(4):
                s = s + pad[:, j, :, e]
        lanes = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ d]
    assert s.dtype == np.float32 and (np.isnan(s[:, 0]) | (s == s[:, :1]).all(axis=1)).all()
    return s[:, 0]


def quantize(x):
    """fp32 rows [N, D] -> (bits [N, width(D)] uint8, scales [N] float32)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, D = x.shape
    assert 1 <= D <= MAX_DIM
    raw = x.view(np.uint32)
    mag = (raw & np.uint32(0x7fffffff)).view(np.float32)
    bad = ((raw & np.uint32(0x7fffffff)) >= np.uint32(0x7f800000)).any(axis=1)
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        sq = x * x
        assert sq.dtype == np.float32
        sumabs, sumsq = _row_sums(mag), _row_sums(sq)
        scales = (sumsq / sumabs).astype(np.float32)
    zero = bad | ~((sumabs > 0) & np.isfinite(sumabs) & np.isfinite(sumsq))
    scales = np.where(bad, np.float32(np.nan), np.where(zero, np.float32(0), scales)).astype(np.float32)
    on = np.zeros((N, width(D) * 8), bool)
    on[:, :D] = (raw >> np.uint32(31)) == 0
    on[zero] = False
    return np.packbits(on, axis=1, bitorder='little'), scales


def signs(bits, D):
    """the stored rows as +-1, int64 [N, D]"""
    on = np.unpackbits(np.asarray(bits, np.uint8), axis=1, bitorder='little')[:, :D]
    return 2 * on.astype(np.int64) - 1


def dot(qcodes, bits, D):
    """t of every pair as int64 [Q, N], exact; |t| <= 127 * D < 2^24 asserted"""
    qc = np.asarray(qcodes, np.int8)[:, :D].astype(np.float64)
    t = (qc @ signs(bits, D).astype(np.float64).T).astype(np.int64)       # exact in fp64: |t| < 2^24 << 2^53
    assert (np.abs(qc).sum(axis=1) < 2.0 ** 24).all() and (np.abs(t) < 2 ** 24).all()
    return t


def score(qcodes, qscales, bits, bscales, D):
    """((float)t * sq[q]) * sb[n], every intermediate fp32"""
    sq, sb = np.asarray(qscales, np.float32), np.asarray(bscales, np.float32)
    t = dot(qcodes, bits, D).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        s = (t * sq[:, None]) * sb[None, :]
    assert s.dtype == np.float32
    return s


def search(q, b, k, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): dir_topk's total order on the scores of int8 queries against sign-bit rows"""
    D = q.shape[1]
    return topk_ref_rows(score(*quantize_i8(q), *quantize(b), D), k, exclude=exclude)


def rerank_sets():
    """fp4_ref's inputs: the queries [33, 200] and the database [3000, 200] of the re-rank tests"""
    return synth_descriptors(5, 33, 200), synth_descriptors(6, 3000, 200)

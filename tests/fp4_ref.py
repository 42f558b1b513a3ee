"""numpy restatement of the fp4 descriptor index (include/dir_engine.h: dir_quantize_rows_fp4, dir_similarity_fp4), for the
fp4 tests.  The definition is in integer operations on the exponent field and exact multiplications by powers of two, and
a score is an exact sum, so the device results are compared bit for bit:

    f_b = exponent field of the largest |x_k| of block b (32 consecutive k);  F = max_b f_b;  m_b = max(f_b, F - 2)
    exps[b] = 127 + m_b - F;  y_k = |x_k| * 2^(129 - m_b);  code_k = nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the
    even code, saturating;  nibble = sign : code, +0 for a value that rounds to zero;  scale = 2^(F - 129)
    score[q][n] = (acc * sq[q]) * sb[n],  acc = sum_k a_k b_k of the values code * 2^(exps - 127)
"""
import numpy as np

from synth import synth_descriptors
from topk_ref import topk_ref_rows

MAX_DIM = 7281                                      # 36 * 64 * 7281 < 2^24 <= 36 * 64 * 7282
GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32)
GRID2 = np.array([0, 1, 2, 3, 4, 6, 8, 12], np.int64)          # twice the grid: integers


def widths(D):
    """(bytes of codes, block bytes) of a stored row: D rounded up to 64, halved; 8 * ceil(D / 256)"""
    return (D + 63) // 64 * 32, (D + 255) // 256 * 8


def _pow2(field):
    """the fp32 number whose exponent field is `field` (1 .. 254): 2^(field - 127)"""
    return (np.asarray(field, np.uint32) << np.uint32(23)).view(np.float32)


def round_codes(y):
    """y >= 0 fp32 -> the 3-bit e2m1 code of the nearest grid value, a midpoint to the even code, saturating at 6"""
    y = np.asarray(y, np.float32)
    return ((y > 0.25).astype(np.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5)).astype(np.uint8)


def quantize(x):
    """fp32 rows [N, D] -> (codes [N, ldc] uint8, exps [N, lde] uint8, scales [N] float32), (ldc, lde) = widths(D)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, D = x.shape
    assert 1 <= D <= MAX_DIM
    ldc, lde = widths(D)
    nb = (D + 31) // 32
    mag = np.zeros((N, nb * 32), np.uint32)
    mag[:, :D] = x.view(np.uint32) & np.uint32(0x7fffffff)
    neg = np.zeros((N, nb * 32), bool)
    neg[:, :D] = (x.view(np.uint32) >> np.uint32(31)).astype(bool)
    top = mag.max(axis=1)
    bad = top >= np.uint32(0x7f800000)                              # an infinity or a NaN: zero codes, scale NaN
    F = (top >> np.uint32(23)).astype(np.int64)
    zero = bad | (F < 127 - 60)                                     # amax < 2^-60: zero codes, scale +0
    F = np.where(zero, 129, F)                                      # (any valid field: the row's codes are dropped below)
    fb = (mag.reshape(N, nb, 32).max(axis=2) >> np.uint32(23)).astype(np.int64)
    m = np.maximum(fb, F[:, None] - 2)
    m = np.where(zero[:, None], 129, m)
    inv = _pow2(256 - m)                                            # 2^-e_b, e_b = m - 129
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        y = mag.view(np.float32).reshape(N, nb, 32) * inv[:, :, None]
    assert y.dtype == np.float32
    code = round_codes(y).reshape(N, nb * 32)
    nib = np.where(code > 0, code | (neg.astype(np.uint8) << 3), 0).astype(np.uint8)
    nib[zero] = 0
    full = np.zeros((N, ldc * 2), np.uint8)
    full[:, :nb * 32] = nib
    codes = (full[:, 0::2] | (full[:, 1::2] << 4)).astype(np.uint8)
    exps = np.full((N, lde), 127, np.uint8)
    exps[:, :nb] = np.where(zero[:, None], 127, 127 + m - F[:, None])
    scales = np.where(bad, np.float32(np.nan), np.where(zero, np.float32(0), _pow2(np.clip(F - 2, 1, 254)))).astype(np.float32)
    return codes, exps, scales


def integers(codes, exps, D):
    """the stored values of a row times 8, as int64 [N, D]: (twice the grid value) * 2^(exps - 125)"""
    codes, exps = np.asarray(codes, np.uint8), np.asarray(exps, np.uint8)
    nib = np.empty((codes.shape[0], codes.shape[1] * 2), np.uint8)
    nib[:, 0::2], nib[:, 1::2] = codes & 15, codes >> 4
    nib = nib[:, :D]
    e = np.repeat(exps.astype(np.int64), 32, axis=1)[:, :D]
    assert ((e >= 125) & (e <= 127)).all()
    v = GRID2[nib & 7] << (e - 125)
    return np.where(nib & 8, -v, v)


def dequantize(codes, exps, scales, D):
    """fp64 values [N, D] of the stored rows (exact: a few bits times a power of two)"""
    return integers(codes, exps, D).astype(np.float64) / 8 * np.asarray(scales, np.float64)[:, None]


def acc(cq, eq, cb, eb, D):
    """the accumulator of every pair as float32 [Q, N], exact: int64 sums of 64 a_k b_k below 2^24, divided by 64"""
    a, b = integers(cq, eq, D), integers(cb, eb, D)
    s = (a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)      # exact in fp64: |s| < 2^24 << 2^53
    assert (np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64).T < 2.0 ** 24).all()
    out = s.astype(np.float32) / np.float32(64)
    assert (out.astype(np.float64) * 64 == s).all()
    return out


def score(cq, eq, sq, cb, eb, sb, D):
    """(acc * sq[q]) * sb[n], every intermediate fp32."""
    sq, sb = np.asarray(sq, np.float32), np.asarray(sb, np.float32)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        s = (acc(cq, eq, cb, eb, D) * sq[:, None]) * sb[None, :]
    assert s.dtype == np.float32
    return s


def search(q, b, k, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): dir_topk's total order on the scores of the quantised rows"""
    D = q.shape[1]
    return topk_ref_rows(score(*quantize(q), *quantize(b), D), k, exclude=exclude)


def rerank_sets():
    """The queries [33, 200] and the database [3000, 200] of the re-rank tests: tests/test_fp4_cpu.py holds on the
    restatement that a shortlist of 4k gives the exact lists, tests/test_fp4_gpu.py runs the index on them."""
    return synth_descriptors(5, 33, 200), synth_descriptors(6, 3000, 200)

"""numpy restatement of the int8 descriptor index (include/dir_engine.h: dir_quantize_rows_i8, dir_similarity_i8), for the
index tests.  Every step is a single IEEE fp32 operation, as the header defines it, so the device results are compared
bit for bit:

    amax = max_k |x_k|;  scale = amax / 127;  inv = 127 / amax;  code_k = clamp(rint(x_k * inv), -127, 127)
    score[q][n] = ((float)dot_i32 * sq[q]) * sb[n]
"""
import numpy as np

F127 = np.float32(127)


def pad64(D):
    return (D + 63) // 64 * 64


def quantize(x):
    """fp32 rows [N, D] -> (codes [N, D rounded up to 64] int8 with zero padding, scales [N] float32)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    N, D = x.shape
    bad = ~np.isfinite(x).all(axis=1)                              # a NaN or an infinity: zero codes, scale NaN
    amax = np.abs(np.where(bad[:, None], np.float32(0), x)).max(axis=1)
    with np.errstate(divide='ignore', over='ignore', invalid='ignore'):
        scale = amax / F127
        inv = F127 / amax
        zero = bad | ~np.isfinite(inv)                             # amax zero or tiny: zero codes, scale 0
        inv = np.where(zero, np.float32(0), inv).astype(np.float32)
        prod = np.where(zero[:, None], np.float32(0), x) * inv[:, None]
    assert scale.dtype == np.float32 and inv.dtype == np.float32 and prod.dtype == np.float32
    codes = np.zeros((N, pad64(D)), np.int8)
    codes[:, :D] = np.clip(np.rint(prod), -127, 127).astype(np.int8)
    scales = np.where(bad, np.float32(np.nan), np.where(zero, np.float32(0), scale)).astype(np.float32)
    return codes, scales


def dots(cq, cb):
    """The int32 dot products cq . cb^T.  Computed in fp64, where they are exact (|dot| < 2^31 << 2^53) and BLAS does the
    work; tests/test_index_cpu.py pins this to cq.astype(int32) @ cb.astype(int32).T."""
    d = np.asarray(cq, np.float64) @ np.asarray(cb, np.float64).T
    assert (np.abs(d) < 2.0 ** 31).all()
    return d.astype(np.int32)


def score(cq, sq, cb, sb):
    """((float)dot * sq[q]) * sb[n], every intermediate fp32."""
    sq, sb = np.asarray(sq, np.float32), np.asarray(sb, np.float32)
    s = (dots(cq, cb).astype(np.float32) * sq[:, None]) * sb[None, :]
    assert s.dtype == np.float32
    return s

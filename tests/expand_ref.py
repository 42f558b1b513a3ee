"""numpy restatement of dir_expand_lists (include/dir_engine.h, the block above its declaration): alpha query expansion /
database augmentation from neighbour lists, every step one numpy operation of `dtype` in the stated order - a loop over
the list slots and over a lane's columns, vectorised over rows and lanes - so that in float32 the device's rows can be
compared bit for bit.  powf (a non-integer alpha) is the one step the definition leaves to the library."""
import numpy as np

SPAN, LANES = 1024, 256      # csrc/expand_lists.hip: columns per span, lanes; lane tau owns columns 4 tau .. 4 tau + 3 of a span


def weights(vals, valid, alpha, dtype=np.float32):
    """w [n,k]: vals^alpha - alpha multiplications from 1 for an integer alpha in 0 .. 64, a power otherwise; the vals of an
    empty slot are not read (its weight here is 1 and is never used)"""
    v = np.where(valid, np.asarray(vals, dtype), dtype(1))
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        if float(alpha) == int(alpha) and 0 <= int(alpha) <= 64:
            w = np.ones_like(v)
            for _ in range(int(alpha)):
                w = w * v
            return w
        return np.power(v, dtype(alpha)).astype(dtype)


def lane_sums(acc):
    """p [n,256]: lane tau's chain p = p + acc_d * acc_d over its columns d, (d mod 1024) / 4 == tau, in ascending d from +0"""
    n, D = acc.shape
    p = np.zeros((n, LANES), acc.dtype)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        for s0 in range(0, D, SPAN):
            for e in range(4):
                cols = np.arange(s0 + e, min(D, s0 + SPAN), 4)      # lane tau's column is cols[tau]
                a = acc[:, cols]
                p[:, :len(cols)] = p[:, :len(cols)] + a * a
    return p


def expand_lists_ref(descs, db, idx, vals, alpha, dtype=np.float32):
    """out [n,D]: acc = descs; for t ascending with idx[:, t] >= 0: acc = acc + (db[idx[:, t]] * w_t); acc = acc * (1 /
    (k + 1)); the lane sums of squares, their tree s = 128 .. 1, one square root, one division per element."""
    descs, db = np.asarray(descs, dtype), np.asarray(db, dtype)
    idx = np.asarray(idx, np.int64)
    n, D = descs.shape
    k = idx.shape[1]
    valid = idx >= 0
    w = weights(np.asarray(vals).reshape(n, k), valid, alpha, dtype)
    acc = descs.copy()
    with np.errstate(invalid='ignore', over='ignore', under='ignore', divide='ignore'):
        for t in range(k):
            on = valid[:, t]
            if not on.any():
                continue
            rows = db[np.where(on, idx[:, t], 0)]
            prod = rows * w[:, t, None]
            acc = np.where(on[:, None], acc + prod, acc)
        inv = dtype(1) / dtype(k + 1)
        acc = acc * inv
        p = lane_sums(acc)
        s = LANES // 2
        while s >= 1:
            p[:, :s] = p[:, :s] + p[:, s:2 * s]
            s //= 2
        return (acc / np.sqrt(p[:, :1])).astype(dtype)

"""numpy restatement of what dir_topk returns (include/dir_engine.h), for the top-k tests: ONE total order - score
descending, larger id first among equal scores (-0 == +0), NaN after every number and by descending id among NaNs - cut
at k, with (-1, NaN) in the slots a short row cannot fill.  On a NaN-free row it is np.argsort(row, kind='stable')[::-1]
(tests/test_topk_cpu.py pins that, and the count dir_rank_counts gives)."""
import numpy as np


def topk_ref(row, k, ids=None, exclude=-1):
    """(idx [k] int32, vals [k] float32) of one row.  ids: the id of every column (None = the column), -1 = a hole;
    exclude: the id that is left out (-1 = none).  vals carries the stored bits of the picked scores."""
    s = np.asarray(row, np.float32)
    ids = np.arange(len(s), dtype=np.int64) if ids is None else np.asarray(ids, np.int64)
    cols = np.flatnonzero((ids >= 0) & (ids != exclude))
    sv, iv = s[cols], ids[cols]
    nan = np.isnan(sv)
    order = np.lexsort((iv, np.where(nan, 0, sv) + 0.0, ~nan))[::-1][:k]
    idx = np.full(k, -1, np.int32)
    vals = np.full(k, np.nan, np.float32)
    idx[:len(order)] = iv[order]
    vals[:len(order)] = sv[order]
    return idx, vals


def topk_ref_rows(scores, k, ids=None, exclude=None):
    """topk_ref of every row: (idx [Q,k] int32, vals [Q,k] float32); ids [Q,N] or None, exclude [Q] or None."""
    scores = np.asarray(scores, np.float32)
    out = [topk_ref(scores[q], k, None if ids is None else ids[q], -1 if exclude is None else int(exclude[q]))
           for q in range(len(scores))]
    if not out:
        return np.empty((0, k), np.int32), np.empty((0, k), np.float32)
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def bits(a):
    """float32 array -> its bit patterns (so that NaNs and signed zeros compare by what is stored)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)

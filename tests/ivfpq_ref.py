"""numpy float32 restatement of the IVF-PQ index (include/dir_engine.h, the block above dir_ivfpq_scan_cols), built on the
restatements of its parts: tests/ivf_ref.py (assignment, probing, the list-major order), tests/pq_ref.py (encoding and the
tables), tests/index_ref.py and tests/topk_ref.py.  Every step is one float32 numpy operation in the stated order, so -
given the centroids and the codebooks - the device's store, coarse terms, scores and lists are compared bit for bit."""
import numpy as np

import index_ref
import ivf_ref
import pq_ref
from topk_ref import topk_ref_rows


def residuals(x, centroids, lists):
    """r [N, D] float32: x_d - centroids[list][d], one subtraction per element against the fp32 centroid"""
    x, c = np.asarray(x, np.float32), np.asarray(centroids, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        r = x - c[np.asarray(lists, np.int64)]
    assert r.dtype == np.float32
    return r


def base(q, centroids, M, probe=None):
    """The coarse terms: s_m = (((+0 + q_{m,0} c_{m,0}) + q_{m,1} c_{m,1}) + ...) over the dsub columns of sub-space m, then
    (((+0 + s_0) + s_1) + ...), m ascending.  probe None: [Q, nlist], the term of every list; probe [Q, nprobe]: the term
    of every slot, NaN for a slot of -1."""
    q, c = np.asarray(q, np.float32), np.asarray(centroids, np.float32)
    D = q.shape[1]
    if M < 1 or D % M or c.shape[1] != D:
        raise ValueError('M dividing the width of queries and centroids expected')
    dsub = D // M
    out = np.zeros((len(q), len(c)), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(M):
            s = np.zeros((len(q), len(c)), np.float32)
            for d in range(m * dsub, (m + 1) * dsub):
                s = s + q[:, d, None] * c[None, :, d]
            out = out + s
    assert out.dtype == np.float32
    if probe is None:
        return out
    probe = np.asarray(probe)
    picked = np.take_along_axis(out, np.maximum(probe, 0).astype(np.int64), axis=1) if len(c) else np.zeros(probe.shape, np.float32)
    return np.where(probe >= 0, picked, np.float32(np.nan)).astype(np.float32)


def scan(tables, start, codes):
    """scores [Q, N] float32: (((start[q][n] + lut[q][0][code[n][0]]) + lut[q][1][code[n][1]]) + ...), m ascending; start
    [Q, N]: the coarse term of query q for the list of row n"""
    tables, codes = np.asarray(tables, np.float32), np.asarray(codes)
    acc = np.array(start, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(tables.shape[1]):
            acc = acc + tables[:, m, :][:, codes[:, m].astype(np.int64)]
    assert acc.dtype == np.float32
    return acc


def build(x, centroids, codebooks):
    """the list-major store of the rows of x: dict(codes [N, M] uint8, ids, list_off, lists) - ivf_ref.build's order (a
    stable sort by list, so ids ascend inside a list), the codes those of the residuals; `lists` is the list of every
    row in ADD order"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    codes = pq_ref.encode(residuals(x, centroids, lists), codebooks)
    order = np.argsort(lists, kind='stable')
    list_off = np.searchsorted(lists[order], np.arange(len(centroids) + 1)).astype(np.int32)
    return dict(codes=codes[order], ids=order.astype(np.int32), list_off=list_off, lists=lists)


def flat_scores(q, x, centroids, codebooks):
    """(scores [Q, N] of every query against every row IN ADD ORDER, each from the coarse term of the row's own list; the
    list of every row)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    M = np.asarray(codebooks).shape[0]
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    codes = pq_ref.encode(residuals(x, centroids, lists), codebooks)
    start = base(q, centroids, M)[:, lists.astype(np.int64)]
    return scan(pq_ref.lut(q, codebooks), start, codes), lists


def search(q, x, centroids, codebooks, k, nprobe, exclude=None, flat=None):
    """(idx [Q,k] int32, vals [Q,k] float32): topk_ref of the flat score matrix with every row outside the probed lists of
    its query masked out (id -1).  flat: flat_scores(q, x, centroids, codebooks), when the caller has it already"""
    scores, lists = flat_scores(q, x, centroids, codebooks) if flat is None else flat
    probed = ivf_ref.probe(*index_ref.quantize(q), centroids, nprobe)
    ids = np.where((lists[None, :, None] == probed[:, None, :]).any(axis=2), np.arange(len(lists), dtype=np.int32)[None, :], -1)
    return topk_ref_rows(scores, k, ids=ids.astype(np.int32), exclude=exclude)


def train_codebooks(x, M, iters=10, seed=0):
    """PQIndex.train's Lloyd iterations in numpy -> codebooks [M, 256, D / M] float32 (the sums in numpy's fp32 order:
    close to the device's, not its bits).  The start: rows np.sort(RandomState(seed).choice(n, 256, replace=False))."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, D = x.shape
    if n < 256 or D % M or not np.isfinite(x).all():
        raise ValueError('at least 256 finite rows of a width M divides expected')
    dsub = D // M
    first = np.sort(np.random.RandomState(seed).choice(n, 256, replace=False))
    codebooks = np.ascontiguousarray(x[first].reshape(256, M, dsub).transpose(1, 0, 2))
    for _ in range(iters):
        codes = pq_ref.encode(x, codebooks)
        for m in range(M):
            sub = x[:, m * dsub:(m + 1) * dsub]
            for j in np.unique(codes[:, m]):
                members = sub[codes[:, m] == j]
                codebooks[m, j] = members.sum(axis=0, dtype=np.float32) / np.float32(len(members))
    return codebooks


def train(x, nlist, M, iters=10, seed=0):
    """(centroids, codebooks): ivf_ref.train, then train_codebooks on the residuals of the same rows to the final centroids"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    centroids = ivf_ref.train(x, nlist, iters=iters, seed=seed)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    return centroids, train_codebooks(residuals(x, centroids, lists), M, iters=iters, seed=seed)

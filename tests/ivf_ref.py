"""numpy restatement of the inverted-file int8 index (include/dir_engine.h: assignment, probing, search, training), for the
IVF tests.  Everything but the sums of a training step is defined through the quantised score of tests/index_ref.py and
the order of tests/topk_ref.py, so - given the centroids - the lists of a search are compared with the device bit for bit."""
import numpy as np

import index_ref
from topk_ref import topk_ref_rows


def centroid_scores(codes, scales, centroids):
    """the quantised scores [rows, nlist] of coded rows against the quantised centroids"""
    cc, cs = index_ref.quantize(centroids)
    D = centroids.shape[1]
    return index_ref.score(codes[:, :D], scales, cc[:, :D], cs)


def assign(codes, scales, centroids):
    """the list of every coded row [n] int32: the best centroid under topk_ref's order (score descending, the larger
    list among equal scores, NaN last - a zero row and a non-finite row go to list nlist - 1)"""
    return topk_ref_rows(centroid_scores(codes, scales, centroids), 1)[0][:, 0]


def probe(qcodes, qscales, centroids, nprobe):
    """the lists of every coded query [Q, nprobe] int32, best first"""
    return topk_ref_rows(centroid_scores(qcodes, qscales, centroids), nprobe)[0]


def build(x, centroids):
    """the list-major store of the rows of x: dict(codes, scales, ids, list_off, lists) - a stable sort by list, so ids
    ascend inside a list; `lists` is the list of every row in ADD order"""
    codes, scales = index_ref.quantize(x)
    lists = assign(codes, scales, centroids)
    order = np.argsort(lists, kind='stable')
    list_off = np.searchsorted(lists[order], np.arange(len(centroids) + 1)).astype(np.int32)
    return dict(codes=codes[order], scales=scales[order], ids=order.astype(np.int32), list_off=list_off, lists=lists)


def search(q, x, centroids, k, nprobe, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): topk_ref of the flat quantised scores with every row outside the probed
    lists of its query masked out (id -1)"""
    qc, qs = index_ref.quantize(q)
    bc, bs = index_ref.quantize(x)
    D = x.shape[1]
    scores = index_ref.score(qc[:, :D], qs, bc[:, :D], bs)
    lists = assign(bc, bs, centroids)
    probed = probe(qc, qs, centroids, nprobe)
    ids = np.where((lists[None, :, None] == probed[:, None, :]).any(axis=2), np.arange(len(x), dtype=np.int32)[None, :], -1)
    return topk_ref_rows(scores, k, ids=ids.astype(np.int32), exclude=exclude)


def l2norm_rows(x, eps=np.float32(1e-12)):
    """ops.l2norm_rows_: x[i] / max(||x[i]||, eps), fp32"""
    x = np.asarray(x, np.float32)
    norm = np.sqrt((x * x).sum(axis=1, dtype=np.float32))
    return (x / np.maximum(norm, eps)[:, None]).astype(np.float32)


def train_sample(x, nlist, seed=0, max_rows=None):
    """(the training sample, the rows of it that start as centroids)"""
    n = len(x)
    max_rows = 256 * nlist if max_rows is None else max_rows
    if n < nlist or max_rows < nlist or not np.isfinite(x).all():
        raise ValueError('finite training data of at least nlist rows expected')
    if n > max_rows:
        x = x[np.sort(np.random.RandomState(seed).choice(n, max_rows, replace=False))]
    return x, np.sort(np.random.RandomState(seed).choice(len(x), nlist, replace=False))


def train(x, nlist, iters=10, seed=0, max_rows=None):
    """spherical Lloyd iterations -> centroids [nlist, D] float32 (the sums in numpy's fp32 order: close to the device's,
    not its bits)"""
    x, first = train_sample(np.ascontiguousarray(x, dtype=np.float32), nlist, seed, max_rows)
    centroids = x[first].copy()
    codes, scales = index_ref.quantize(x)
    for _ in range(iters):
        lists = assign(codes, scales, centroids)
        sums = np.zeros_like(centroids)
        for l in range(nlist):
            sums[l] = x[lists == l].sum(axis=0, dtype=np.float32)
        centroids = np.where((np.bincount(lists, minlength=nlist) == 0)[:, None], centroids, l2norm_rows(sums))
    return centroids.astype(np.float32)


def objective(x, centroids, lists):
    """the mean exact cosine of a row to the centroid of its list (fp64)"""
    x, c = np.asarray(x, np.float64), np.asarray(centroids, np.float64)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    c = c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-300)
    return float((x * c[lists]).sum(axis=1).mean())


def lloyd64(x, first, iters=10):
    """the same iterations in fp64 with exact assignments (argmax of the cosines) from the same start -> (centroids, lists
    of the rows to the final centroids)"""
    x = np.asarray(x, np.float64)
    c = x[first].copy()
    for _ in range(iters):
        lists = (x @ c.T).argmax(axis=1)
        for l in range(len(c)):
            if (lists == l).any():
                s = x[lists == l].sum(axis=0)
                c[l] = s / np.linalg.norm(s)
    return c, (x @ c.T).argmax(axis=1)

"""numpy restatement of the inverted file over sign-bit rows (include/dir_engine.h: dir_ivf_scan_bin, index.IVFBinaryIndex),
for its tests.  It is a composition of two restatements that exist: the coarse side - assignment and probing by the quantised
int8 score - is tests/ivf_ref.py's, the rows and their scores are tests/bin_ref.py's.  A score is an exact integer times two
fp32 factors, so - given the centroids - the store and the lists of a search are compared with the device bit for bit."""
import numpy as np

import bin_ref
import index_ref
import ivf_ref
from topk_ref import topk_ref_rows


def build(x, centroids):
    """the list-major store of the rows of x: dict(codes, scales, ids, list_off, lists) - ivf_ref.assign on the int8 codes,
    then a stable sort of bin_ref.quantize's two arrays by list, so ids ascend inside a list; `lists` is the list of every
    row in ADD order"""
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    codes, scales = bin_ref.quantize(x)
    order = np.argsort(lists, kind='stable')
    list_off = np.searchsorted(lists[order], np.arange(len(centroids) + 1)).astype(np.int32)
    return dict(codes=codes[order], scales=scales[order], ids=order.astype(np.int32), list_off=list_off, lists=lists)


def search(q, x, centroids, k, nprobe, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): topk_ref of the flat sign-bit scores with every row outside the probed lists
    of its query masked out (id -1); the lists of a row and of a query come from their int8 codes, which score the rows too"""
    D = x.shape[1]
    qc, qs = index_ref.quantize(q)
    scores = bin_ref.score(qc, qs, *bin_ref.quantize(x), D)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    probed = ivf_ref.probe(qc, qs, centroids, nprobe)
    ids = np.where((lists[None, :, None] == probed[:, None, :]).any(axis=2), np.arange(len(x), dtype=np.int32)[None, :], -1)
    return topk_ref_rows(scores, k, ids=ids.astype(np.int32), exclude=exclude)

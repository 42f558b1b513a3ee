"""numpy restatement of the inverted file over fp4 codes (include/dir_engine.h: dir_ivf_scan_fp4, index.IVFFp4Index), for
its tests.  It is a composition of two restatements that exist: the coarse side - assignment and probing by the quantised
int8 score - is tests/ivf_ref.py's, the rows and their scores are tests/fp4_ref.py's.  A score is an exact sum times two
powers of two, so - given the centroids - the store and the lists of a search are compared with the device bit for bit."""
import numpy as np

import fp4_ref
import index_ref
import ivf_ref
from topk_ref import topk_ref_rows


def build(x, centroids):
    """the list-major store of the rows of x: dict(codes, exps, scales, ids, list_off, lists) - ivf_ref.assign on the int8
    codes, then a stable sort of fp4_ref.quantize's three arrays by list, so ids ascend inside a list; `lists` is the list
    of every row in ADD order"""
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    codes, exps, scales = fp4_ref.quantize(x)
    order = np.argsort(lists, kind='stable')
    list_off = np.searchsorted(lists[order], np.arange(len(centroids) + 1)).astype(np.int32)
    return dict(codes=codes[order], exps=exps[order], scales=scales[order], ids=order.astype(np.int32), list_off=list_off,
                lists=lists)


def search(q, x, centroids, k, nprobe, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): topk_ref of the flat fp4 scores with every row outside the probed lists of
    its query masked out (id -1); the lists of a row and of a query come from their int8 codes"""
    D = x.shape[1]
    scores = fp4_ref.score(*fp4_ref.quantize(q), *fp4_ref.quantize(x), D)
    lists = ivf_ref.assign(*index_ref.quantize(x), centroids)
    probed = ivf_ref.probe(*index_ref.quantize(q), centroids, nprobe)
    ids = np.where((lists[None, :, None] == probed[:, None, :]).any(axis=2), np.arange(len(x), dtype=np.int32)[None, :], -1)
    return topk_ref_rows(scores, k, ids=ids.astype(np.int32), exclude=exclude)

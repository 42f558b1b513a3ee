"""numpy fp64 restatement of what dir_label_rank computes (include/dir_engine.h), for the label-rank tests: the order-free
form of sklearn's average_precision_score and the best rank of a same-class image under a stable descending argsort.
Written from the definitions, not from the kernel: counts come from np.sort + np.searchsorted and from plain compares."""
import numpy as np


def ap_ref(scores, positive, keep=None):
    """AP = (1/n_pos) * sum over kept positives p of pos_ge(s_p) / all_ge(s_p); -1.0 without a kept positive, NaN when a
    kept score is NaN or infinite.  Tied scores share a threshold and -0 == +0 (float compares)."""
    scores = np.asarray(scores)
    positive = np.asarray(positive, dtype=bool)
    if keep is not None:
        scores, positive = scores[keep], positive[keep]
    if not positive.any():
        return -1.0
    if not np.isfinite(scores).all():
        return float('nan')
    s = scores.astype(np.float64) + 0.0          # -0 -> +0
    every, pos = np.sort(s), np.sort(s[positive])
    all_ge = len(every) - np.searchsorted(every, pos, side='left')
    pos_ge = len(pos) - np.searchsorted(pos, pos, side='left')
    return float(np.sum(pos_ge.astype(np.float64) / all_ge.astype(np.float64)) / len(pos))


def best_rank_ref(scores, correct):
    """Position, under np.argsort(-scores, kind='stable') (score descending, index ascending on ties, NaN after every
    number), of the best-placed item with correct[j]; len(scores) when there is none."""
    scores = np.asarray(scores)
    correct = np.asarray(correct, dtype=bool)
    n = len(scores)
    if not correct.any():
        return n
    idx = np.arange(n)
    nan = np.isnan(scores)
    numbered = correct & ~nan
    if numbered.any():
        m = scores[numbered].max()
        first = idx[numbered & (scores == m)][0]
        with np.errstate(invalid='ignore'):
            return int(np.sum(scores > m) + np.sum((scores == m) & (idx < first)))
    first = idx[correct][0]                      # every image of the class scored NaN
    return int(np.sum(~nan) + np.sum(nan & (idx < first)))


def label_rank_ref(scores, labels, qclass, qself):
    """(ap [Q] float64, best_rank [Q] int64) for score rows [Q, N], class ids labels [N], qclass [Q] (-1 = no image of
    the class), qself [Q] (-1 = the query is not a database image)."""
    scores = np.asarray(scores)
    labels = np.asarray(labels)
    Q, N = scores.shape
    ap, best = np.empty(Q, np.float64), np.empty(Q, np.int64)
    for q in range(Q):
        correct = (labels == qclass[q]) if qclass[q] >= 0 else np.zeros(N, bool)
        keep = np.ones(N, bool)
        if qself[q] >= 0:
            keep[qself[q]] = False
        ap[q] = ap_ref(scores[q], correct, keep)
        best[q] = best_rank_ref(scores[q], correct)
    return ap, best


def csr_tables(labels, C):
    """(class_off [C+1], class_members [N]) int32 of integer class ids in [0, C)."""
    labels = np.asarray(labels)
    members = np.argsort(labels, kind='stable').astype(np.int32)
    off = np.zeros(C + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(labels, minlength=C))
    return off, members

"""numpy float32 restatement of the product-quantised index (include/dir_engine.h, the block above dir_pq_max_m): the
encoding, the tables of a query and the score, every step one float32 numpy operation in the stated order - loops over the
columns of a sub-space and over the sub-spaces, vectorised over rows and centroids - so the device's codes, tables and
scores can be compared bit for bit."""
import numpy as np

from topk_ref import topk_ref_rows


def _split(D, codebooks):
    """(M, dsub) of codebooks [M, 256, dsub] for rows of D values"""
    codebooks = np.asarray(codebooks)
    M, K, dsub = codebooks.shape
    if K != 256 or M * dsub != D:
        raise ValueError('codebooks [M, 256, D / M] expected')
    return M, dsub


def distances(x, codebooks, m):
    """dist [N, 256] float32 of sub-space m: (((+0 + t_0 t_0) + t_1 t_1) + ...), t_d = x_d - c_d, in column order"""
    x, c = np.asarray(x, np.float32), np.asarray(codebooks, np.float32)
    M, dsub = _split(x.shape[1], c)
    dist = np.zeros((len(x), 256), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for d in range(dsub):
            t = x[:, m * dsub + d, None] - c[m, :, d][None, :]
            dist = dist + t * t
    return dist


def encode(x, codebooks):
    """codes [N, M] uint8: best = 0; for j = 1 .. 255: dist_j < dist_best, or dist_best a NaN and dist_j not, moves best to
    j - the smaller j among equal distances, a NaN never chosen over a number, code 0 where every distance is a NaN"""
    x = np.asarray(x, np.float32)
    M, _ = _split(x.shape[1], codebooks)
    codes = np.zeros((len(x), M), np.uint8)
    rows = np.arange(len(x))
    for m in range(M):
        dist = distances(x, codebooks, m)
        best = np.zeros(len(x), np.int64)
        for j in range(1, 256):
            cur = dist[rows, best]
            with np.errstate(invalid='ignore'):
                better = (dist[:, j] < cur) | (np.isnan(cur) & ~np.isnan(dist[:, j]))
            best = np.where(better, j, best)
        codes[:, m] = best
    return codes


def lut(q, codebooks):
    """tables [Q, M, 256] float32: lut[q][m][j] = (((+0 + q_0 c_0) + q_1 c_1) + ...) over the columns of sub-space m"""
    q, c = np.asarray(q, np.float32), np.asarray(codebooks, np.float32)
    M, dsub = _split(q.shape[1], c)
    out = np.zeros((len(q), M, 256), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(M):
            acc = np.zeros((len(q), 256), np.float32)
            for d in range(dsub):
                acc = acc + q[:, m * dsub + d, None] * c[m, :, d][None, :]
            out[:, m] = acc
    return out


def scan(tables, codes):
    """scores [Q, N] float32: (((+0 + lut[q][0][code[n][0]]) + lut[q][1][code[n][1]]) + ...), m ascending"""
    tables, codes = np.asarray(tables, np.float32), np.asarray(codes)
    Q, M, _ = tables.shape
    acc = np.zeros((Q, len(codes)), np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(M):
            acc = acc + tables[:, m, :][:, codes[:, m].astype(np.int64)]
    return acc


def search_ref(q, x, codebooks, k, exclude=None):
    """(idx [Q,k] int32, vals [Q,k] float32): topk_ref of the scores of the queries against the encoded rows of x"""
    return topk_ref_rows(scan(lut(q, codebooks), encode(x, codebooks)), k, exclude=exclude)


def reconstruction_error(x, codebooks, codes):
    """the mean squared distance of a row to the centroids its codes name, fp64"""
    x, c = np.asarray(x, np.float64), np.asarray(codebooks, np.float64)
    M, dsub = _split(x.shape[1], c)
    err = 0.0
    for m in range(M):
        r = x[:, m * dsub:(m + 1) * dsub] - c[m, np.asarray(codes)[:, m].astype(np.int64)]
        err += (r * r).sum()
    return err / len(x)

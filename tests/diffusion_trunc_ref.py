"""numpy restatement of the truncated diffusion (include/dir_engine.h, the block above dir_diffusion_subgraph): the
subgraph of every query's candidate list, its solve - tests/diffusion_ref.py's solve_ref on the local graph, one column a
query - and the spread of the list scores over score rows.  In float32 the device's numbers are compared bit for bit."""
import numpy as np

from diffusion_ref import power, solve_ref


def live_candidates(cidx, N):
    """[Q,T] bool: the id in [0, N) and no earlier slot of the list holds it"""
    cidx = np.asarray(cidx, np.int64)
    live = (cidx >= 0) & (cidx < N)
    for a in range(1, cidx.shape[1]):
        live[:, a] &= ~(cidx[:, :a] == cidx[:, a:a + 1]).any(axis=1)
    return live


def subgraph_ref(idx, S, cidx, cvals, kq, gamma=3, one_hot=False, dtype=np.float32):
    """(cid [Q,T] int32, lidx [Q,k,T] int32, lw [Q,k,T], y [Q,T]): cid the id of a live candidate, else -1; slot t of a
    live candidate a with i = cid[a]: the local number b of j = idx[i][t] and S[i][t] when S[i][t] != 0, 0 <= j < N and j
    is a live candidate, else -1 / +0; y = cvals^gamma over the live ones of the first kq with a score > 0, or 1 at a live
    candidate 0 with one_hot"""
    idx, S = np.asarray(idx, np.int64), np.asarray(S, dtype)
    cidx = np.asarray(cidx, np.int64)
    N, k = idx.shape
    Q, T = cidx.shape
    live = live_candidates(cidx, N)
    cid = np.where(live, cidx, -1).astype(np.int32)
    lidx = np.full((Q, k, T), -1, np.int32)
    lw = np.zeros((Q, k, T), dtype)
    y = np.zeros((Q, T), dtype)
    for q in range(Q):
        where = np.full(N, -1, np.int64)                      # global id -> local number of its live candidate
        rows = np.flatnonzero(live[q])
        where[cidx[q, rows]] = rows
        if len(rows) and k:
            j, s = idx[cidx[q, rows]], S[cidx[q, rows]]       # [rows, k]
            inside = (j >= 0) & (j < N) & (s != 0)
            b = np.where(inside, where[np.where(inside, j, 0)], -1)
            lidx[q][:, rows] = b.T
            lw[q][:, rows] = np.where(b >= 0, s, dtype(0)).T
        if one_hot:
            if live[q, 0]:
                y[q, 0] = 1
        else:
            head = min(kq, T)
            v = np.asarray(cvals[q, :head], dtype)
            with np.errstate(invalid='ignore'):
                ok = live[q, :head] & (v > 0)
            y[q, :head] = np.where(ok, power(np.where(ok, v, dtype(1)), gamma, dtype), dtype(0))
    return cid, lidx, lw, y


def solve_local_ref(lidx, lw, y, cid, alpha, iters, dtype=np.float32):
    """f [Q,T]: solve_ref on every query's local graph with its one seed column; NaN where cid < 0 (cid None: nowhere)"""
    Q, k, T = lidx.shape
    f = np.zeros((Q, T), dtype)
    for q in range(Q):
        f[q] = solve_ref(np.ascontiguousarray(lidx[q].T), np.ascontiguousarray(lw[q].T), y[q][:, None], alpha, iters, dtype)[:, 0]
    if cid is not None:
        f[np.asarray(cid) < 0] = np.nan
    return f


def spread_ref(scores, cid, f):
    """[Q,N]: every score minus 4, then a live candidate's column = f > -2 ? f : -2 (a NaN f: -2)"""
    out = (np.asarray(scores, np.float32) - np.float32(4)).astype(np.float32)
    N = out.shape[1]
    for q in range(out.shape[0]):
        on = (cid[q] >= 0) & (cid[q] < N)
        with np.errstate(invalid='ignore'):
            v = np.where(f[q] > -2, f[q], np.float32(-2)).astype(np.float32)
        out[q, cid[q][on]] = v[on]
    return out


def local_dense(lidx_q, lw_q):
    """the [T,T] matrix of one query's local graph [k,T]"""
    k, T = lidx_q.shape
    A = np.zeros((T, T), lw_q.dtype)
    for t in range(k):
        on = lidx_q[t] >= 0
        A[np.flatnonzero(on), lidx_q[t][on]] = lw_q[t][on]
    return A


def truncated_ref(q, b, graph, trunc, kq, gamma, alpha, iters, same_set=False, lists=None):
    """(cid, f, dense scores) of the whole route on the host: candidates = the exact fp32 lists (or `lists`), with the
    query's own row in front for same_set"""
    from diffusion_ref import exact_lists
    idx, S = graph
    if lists is None:
        if same_set:
            oi, ov = exact_lists(q, b, trunc - 1, True)
            lists = (np.concatenate([np.arange(len(q), dtype=np.int32)[:, None], oi], axis=1),
                     np.concatenate([np.ones((len(q), 1), np.float32), ov], axis=1))
        else:
            lists = exact_lists(q, b, trunc, False)
    cid, lidx, lw, y = subgraph_ref(idx, S, lists[0], lists[1], kq, gamma, one_hot=same_set)
    f = solve_local_ref(lidx, lw, y, cid, alpha, iters)
    dense = spread_ref(np.asarray(q, np.float32) @ np.asarray(b, np.float32).T, cid, f)
    return cid, f, dense

"""numpy restatement of dir_knn_graph, dir_diffusion_seed and dir_diffusion_solve (include/dir_engine.h, the block above
their declarations): every step one numpy operation of `dtype` in the stated order, vectorised over rows and columns, so
that in float32 the device's numbers can be compared bit for bit.  powf (a non-integer gamma) is the one step the
definition leaves to the library.  two_rings() is the small retrieval problem where plain ranking fails and a walk along
the graph succeeds; mean_ap() scores a ranking of it."""
import numpy as np

SLAB, CHAINS = 256, 64      # csrc/diffusion.hip: rows of a slab of a dot product, chains of a slab (row r: chain r mod 64)

_QUIET = dict(invalid='ignore', over='ignore', under='ignore', divide='ignore')


def power(v, gamma, dtype=np.float32):
    """v^gamma: gamma multiplications from 1 for an integer gamma in 0 .. 64, a power otherwise"""
    v = np.asarray(v, dtype)
    with np.errstate(**_QUIET):
        if float(gamma) == int(gamma) and 0 <= int(gamma) <= 64:
            w = np.ones_like(v)
            for _ in range(int(gamma)):
                w = w * v
            return w
        return np.power(v, dtype(gamma)).astype(dtype)


def live_slots(idx, vals, N, self_test):
    """[n,k] bool: the id in [0, N), not the row itself (self_test), no earlier slot of the row holds it, the score > 0"""
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    with np.errstate(invalid='ignore'):
        live = (idx >= 0) & (idx < N) & (np.asarray(vals) > 0)
    if self_test:
        live &= idx != np.arange(n)[:, None]
    for t in range(1, k):
        live[:, t] &= ~(idx[:, :t] == idx[:, t:t + 1]).any(axis=1)
    return live


def knn_graph_ref(idx, vals, gamma=3, dtype=np.float32):
    """S [N,k]: a(i,t) = min(w(i,t), w(j,t')) over the mutual live slots, deg the chain over t, dinv = 1 / sqrt(deg),
    S = a * (dinv[i] * dinv[j])"""
    idx = np.asarray(idx, np.int64)
    N, k = idx.shape
    live = live_slots(idx, vals, N, True)
    w = power(np.where(live, np.asarray(vals, dtype), dtype(1)), gamma, dtype)
    a = np.zeros((N, k), dtype)
    for i in range(N):
        for t in range(k):
            if not live[i, t]:
                continue
            j = idx[i, t]
            back = np.flatnonzero((idx[j] == i) & live[j])
            if len(back):
                a[i, t] = min(w[i, t], w[j, back[0]])
    with np.errstate(**_QUIET):
        deg = np.zeros(N, dtype)
        for t in range(k):
            deg = deg + a[:, t]
        dinv = np.where(deg > 0, dtype(1) / np.sqrt(np.where(deg > 0, deg, dtype(1))), dtype(0)).astype(dtype)
        on = a != 0
        pair = dinv[:, None] * dinv[np.where(on, idx, 0)]
        return np.where(on, a * pair, dtype(0)).astype(dtype)


def seed_ref(qidx, qvals, N, gamma=3, dtype=np.float32):
    """Y [N,Q]: zero except Y[qidx[q][t]][q] = qvals[q][t]^gamma for ids in [0, N) with a score > 0, t ascending (a later
    slot that names the same row overwrites an earlier one)"""
    qidx = np.asarray(qidx, np.int64)
    Q, kq = qidx.shape
    Y = np.zeros((N, Q), dtype)
    with np.errstate(invalid='ignore'):
        ok = (qidx >= 0) & (qidx < N) & (np.asarray(qvals) > 0)
    w = power(np.where(ok, np.asarray(qvals, dtype), dtype(1)), gamma, dtype)
    for q in range(Q):
        for t in range(kq):
            if ok[q, t]:
                Y[qidx[q, t], q] = w[q, t]
    return Y


def dot_ref(u, v):
    """dot of every column [Q]: slabs of 256 rows; chain c of a slab adds the products of its rows c, c + 64, .. in ascending
    order from +0; the tree s = 32 .. 1 over the chains; the slab partials added in ascending slab order from +0"""
    N, Q = u.shape
    dtype = u.dtype.type
    slabs = (N + SLAB - 1) // SLAB
    with np.errstate(**_QUIET):
        prod = np.zeros((slabs * SLAB, Q), u.dtype)
        prod[:N] = u * v
        there = (np.arange(slabs * SLAB) < N).reshape(slabs, SLAB // CHAINS, CHAINS)
        prod = prod.reshape(slabs, SLAB // CHAINS, CHAINS, Q)
        chain = np.zeros((slabs, CHAINS, Q), u.dtype)
        for m in range(SLAB // CHAINS):
            chain = np.where(there[:, m, :, None], chain + prod[:, m], chain)
        s = CHAINS // 2
        while s >= 1:
            chain[:, :s] = chain[:, :s] + chain[:, s:2 * s]
            s //= 2
        d = np.zeros(Q, u.dtype)
        for b in range(slabs):
            d = d + chain[b, 0]
    return d.astype(dtype)


def apply_ref(idx, S, p):
    """g [N,Q]: the chain g = g + S[i][t] * p[idx[i][t]] over t ascending, the slots with an id outside [0, N) or S == 0 skipped"""
    N, k = idx.shape
    g = np.zeros_like(p)
    with np.errstate(**_QUIET):
        for t in range(k):
            on = (idx[:, t] >= 0) & (idx[:, t] < N) & (S[:, t] != 0)
            if not on.any():
                continue
            rows = p[np.where(on, idx[:, t], 0)]
            g = np.where(on[:, None], g + S[:, t, None] * rows, g)
    return g


def solve_ref(idx, S, Y, alpha, iters, dtype=np.float32):
    """F [N,Q]: `iters` conjugate-gradient iterations on (I - alpha S) f = y for every column, in the header's order"""
    idx = np.asarray(idx, np.int64)
    S, Y = np.asarray(S, dtype), np.asarray(Y, dtype)
    alpha = dtype(alpha)
    x = np.zeros_like(Y)
    if iters <= 0 or Y.size == 0:
        return x
    r, p = Y.copy(), Y.copy()
    rr = dot_ref(r, r)
    with np.errstate(**_QUIET):
        for _ in range(iters):
            ap = p - alpha * apply_ref(idx, S, p)
            pap = dot_ref(p, ap)
            a = np.where(pap > 0, rr / np.where(pap > 0, pap, dtype(1)), dtype(0)).astype(dtype)
            x = x + a * p
            r = r - a * ap
            rn = dot_ref(r, r)
            b = np.where(rr > 0, rn / np.where(rr > 0, rr, dtype(1)), dtype(0)).astype(dtype)
            p = r + b * p
            rr = rn
    return x


def dense_graph(idx, S):
    """the [N,N] matrix of a graph in the list layout (slots with S == 0 left out)"""
    idx = np.asarray(idx, np.int64)
    N, k = idx.shape
    A = np.zeros((N, N), S.dtype)
    for i in range(N):
        for t in range(k):
            if S[i, t] != 0:
                A[i, idx[i, t]] = S[i, t]
    return A


def two_rings(n_per=200, D=8):
    """(qdescs [16,D], bdescs [384,D], positives): unit vectors on two latitude circles of the unit sphere (0.35 and 0.60
    rad) in the first three dimensions, n_per points each at longitudes (j + 0.5 c) 2 pi / n_per for circle c; every 25th
    point is a query and leaves the database; the positives of a query are the database points of its own circle.  Far
    points of the same circle score below near points of the other one, so plain ranking fails where a walk succeeds."""
    pts = np.zeros((2 * n_per, D), np.float64)
    circle = np.repeat(np.arange(2), n_per)
    for c, lat in enumerate((0.35, 0.60)):
        lon = (np.arange(n_per) + 0.5 * c) * 2 * np.pi / n_per
        pts[c * n_per:(c + 1) * n_per, 0] = np.cos(lat) * np.cos(lon)
        pts[c * n_per:(c + 1) * n_per, 1] = np.cos(lat) * np.sin(lon)
        pts[c * n_per:(c + 1) * n_per, 2] = np.sin(lat)
    isq = np.arange(2 * n_per) % 25 == 0
    q, b = pts[isq].astype(np.float32), pts[~isq].astype(np.float32)
    bc = circle[~isq]
    positives = [np.flatnonzero(bc == c) for c in circle[isq]]
    return q, b, positives


def mean_ap(scores, positives):
    """the mean over the queries of the average precision of ranking the columns of a score row in descending order"""
    aps = []
    for row, pos in zip(np.asarray(scores), positives):
        order = np.argsort(-row, kind='stable')
        hit = np.isin(order, pos)
        ranks = np.flatnonzero(hit) + 1
        aps.append(float(np.mean(np.arange(1, len(ranks) + 1) / ranks)))
    return float(np.mean(aps))


DEAD_SLOTS = {'hole': (2, 3), 'range': (3, 2), 'self': (4, 4), 'dup': (5, 5), 'zero': (6, 1), 'neg': (7, 0), 'nan': (8, 1)}
ISOLATED_ROW = 9


def planted_lists(N, k, seed):
    """(idx [N,k] int32, vals [N,k] float32, {kind: (i, t)}): self-set lists where slot t of row i names row i + 1, i - 1,
    i + 2, i - 2, .. (mod N), so the slots pair up into mutual edges and the last slot of an odd k is one-sided (k = 1:
    rows pair up as i ^ 1); random scores in (0.1, 1); then a dead slot of every kind planted where k has room - a -1
    hole with a NaN score, an id far out of range, the row itself, a later duplicate, a score of 0, a negative one, a
    NaN - at DEAD_SLOTS (the slot taken mod k) and ISOLATED_ROW with no positive score at all.  N >= 10."""
    r = np.random.RandomState(seed)
    step = np.array([(t // 2 + 1) * (1 if t % 2 == 0 else -1) for t in range(k)])
    idx = ((np.arange(N)[:, None] + step[None, :]) % N).astype(np.int32)
    if k == 1:
        idx[:, 0] = np.where((np.arange(N) ^ 1) < N, np.arange(N) ^ 1, -1)
    vals = r.uniform(0.1, 1.0, (N, k)).astype(np.float32)
    dead = {}
    for kind, (i, t) in DEAD_SLOTS.items():
        t %= k
        if kind == 'dup' and t == 0:
            continue
        dead[kind] = (i, t)
        if kind == 'hole':
            idx[i, t], vals[i, t] = -1, np.nan
        elif kind == 'range':
            idx[i, t] = N + (1 << 20)
        elif kind == 'self':
            idx[i, t] = i
        elif kind == 'dup':
            idx[i, t] = idx[i, 0]
        else:
            vals[i, t] = {'zero': 0.0, 'neg': -0.5, 'nan': np.nan}[kind]
    vals[ISOLATED_ROW, :] = -1.0
    return idx, vals, dead


def exact_lists(q, db, k, same_set):
    """the stable-argsort lists of the fp32 scores, best first: (idx [n,k] int32, vals [n,k] float32)"""
    from topk_ref import topk_ref_rows
    scores = np.asarray(q, np.float32) @ np.asarray(db, np.float32).T
    return topk_ref_rows(scores, k, exclude=np.arange(len(q)) if same_set else None)

"""Device-side ranking + AP for revisitop-style datasets and, further down, for class-labelled ones
(build_label_tables / eval_labelled_device: sklearn AP and top-k hits, the score matrix made and ranked in row chunks).

Same numbers as `[db.eval_query_AP(q, s) for q, s in enumerate(scores)]`
(dirtorch/test_dir.py:153, dirtorch/datasets/generic.py:196-224) without downloading the Q x N score
matrix or sorting it: one kernel counts, for every listed image of every query, how many database
items rank before it; a second one applies the junk corrections among those few hundred listed images
and sums the AP in fp64 in the reference's order.  Ties rank by descending index (np.argsort(...)[::-1] with a stable order).
"""
import numpy as np
import torch

from . import ops


UNIT_RANGE_BOUND = 60.0     # csrc/sim_split.hip PAIR form: operands in (-64, 64)
UNIT_RANGE_MIN_ROWS = 32768  # ... which only exists on the large-database path


def is_unit_range(*tensors):
    """True when every value lies inside the fp16-pair similarity kernel's range (one abs-max pass per tensor, one
    host sync: call it once per database, not per query batch).  L2-normalised descriptors always qualify."""
    for t in tensors:
        if t.numel():
            lo, hi = torch.aminmax(t)      # (no |t| temporary: the database is 8 GB at config D's sizes)
            if not max(-float(lo), float(hi)) < UNIT_RANGE_BOUND:      # (NaN compares false: not in range)
                return False
    return True


_RANGE_ATTR = '_dirtorch_unit_range'     # (tensor._version, data_ptr, verdict), kept ON the caller's tensor object


def database_is_unit_range(b):
    """is_unit_range(b), remembered ON the database tensor the caller holds: the full pass over an 8 GB database (1.5 ms + a
    host sync) is paid once per tensor OBJECT, not on every query batch.  The verdict is an attribute of that object, so it
    dies with it - a new tensor that the caching allocator places at the same address starts without one (round-5 advice:
    a (data_ptr, shape, version) key could be served to a different upload) - and it carries the version counter and the
    address it was taken at, so an in-place torch update or a .set_() re-checks.  What torch cannot see - a refill through
    raw pointers, e.g. by this library's own kernels - must drop it: forget_unit_range(b), or pass unit_range= explicitly."""
    tag = getattr(b, _RANGE_ATTR, None)
    if tag is not None and tag[0] == b._version and tag[1] == b.data_ptr():
        return tag[2]
    verdict = is_unit_range(b)
    try:
        setattr(b, _RANGE_ATTR, (b._version, b.data_ptr(), verdict))
    except AttributeError:      # (an object that takes no attributes: no caching)
        pass
    return verdict


def forget_unit_range(b):
    """Drop the remembered range verdict of a database tensor whose contents were rewritten behind torch's back."""
    if hasattr(b, _RANGE_ATTR):
        delattr(b, _RANGE_ATTR)


def similarity_device(qdescs, bdescs, unit_range=None):
    """Scores Q.DB^T as a CUDA tensor [Q, N] (common.matmul without the download).  unit_range: True = the caller knows
    both sets are bounded by 60 in magnitude (L2-normalised descriptors: dirtorch/test_dir.py:150) and wants the fp16-pair
    kernel on large databases (ops.similarity); None (default) = look, when the database is large enough for it to matter -
    the DATABASE's verdict is remembered on the caller's own CUDA tensor (database_is_unit_range), only the small query block is checked per call;
    False = never.  Evaluation loops that know their descriptors are L2-normalised pass True."""
    from .utils.common import _dev
    q, b = _dev(qdescs), _dev(bdescs)
    if unit_range is None:
        # the verdict is only REMEMBERED for a database the caller owns as a float32 CUDA tensor (_dev hands that very object
        # back); an ndarray / a CPU or non-fp32 tensor is uploaded into a temporary, which is checked in full and forgotten
        owned = b is bdescs
        unit_range = (b.shape[0] >= UNIT_RANGE_MIN_ROWS and (database_is_unit_range(b) if owned else is_unit_range(b))
                      and is_unit_range(q))
    return ops.similarity(q, b, unit_range=bool(unit_range))


def _mode_lists(groups, classic):
    """[(positives, junk)] per mode, as the reference builds them (generic.py:150-170, 196-224)."""
    if classic:
        return [(groups['ok'], groups['junk'])]
    return [(groups['easy'], groups['junk'] + groups['hard']),
            (groups['easy'] + groups['hard'], groups['junk']),
            (groups['hard'], groups['junk'] + groups['easy'])]


def build_probe_tables(db):
    """Host-side index tables for eval_aps_device, built once per dataset: the union list of listed
    images per query (probe_idx [Q,P], -1 padded) and, per (query, mode), the positions of the mode's
    positives and junk inside that list (CSR).  Duplicates are dropped; an image listed as positive AND
    junk is junk (the reference writes junk last, generic.py:192)."""
    Q = db.nquery
    classic = bool(db.relevants)
    modes = 1 if classic else 3
    rows, pos_off, pos_list, junk_off, junk_list = [], [0], [], [0], []
    for q in range(Q):
        if classic:
            groups = {'ok': list(db.relevants[q]), 'junk': list(db.junk[q])}
        else:
            groups = {'easy': list(db.easy[q]), 'hard': list(db.hard[q]), 'junk': list(db.junk[q])}
        flat = list(dict.fromkeys(i for v in groups.values() for i in v))
        where = {i: k for k, i in enumerate(flat)}
        rows.append(flat)
        for positives, junk in _mode_lists(groups, classic):
            junkset = set(junk)
            pos_list += [where[i] for i in dict.fromkeys(positives) if i not in junkset]
            junk_list += [where[i] for i in sorted(junkset)]
            pos_off.append(len(pos_list))
            junk_off.append(len(junk_list))
    P = max(1, max(len(r) for r in rows))
    probe = -np.ones((Q, P), dtype=np.int32)
    for q, r in enumerate(rows):
        probe[q, :len(r)] = r
    as_dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.int32)).cuda()   # noqa: E731
    return dict(probe=torch.from_numpy(probe).cuda(), pos_off=as_dev(pos_off), pos_list=as_dev(pos_list or [0]),
                junk_off=as_dev(junk_off), junk_list=as_dev(junk_list or [0]), modes=modes, classic=classic)


def eval_aps_device(db, scores, tables=None):
    """scores: CUDA tensor [Q, N].  Returns the list the reference builds: one float per query
    (classic protocol) or one {'easy','medium','hard'} dict per query.  Two kernels: the dense rank
    counts of every listed image (dir_rank_counts, one pass over the score rows) and the junk-corrected
    APs (dir_revisitop_ap); only Q x modes doubles come back to the host."""
    Q, N = scores.shape
    assert Q == db.nquery and N == db.nimg, "scores should have shape (%d, %d)" % (db.nquery, db.nimg)
    t = tables if tables is not None else build_probe_tables(db)
    counts, pscores = ops.rank_counts(scores.contiguous(), t['probe'])
    ap = ops.revisitop_ap(t['probe'], counts, pscores, t['pos_off'], t['pos_list'], t['junk_off'],
                          t['junk_list'], t['modes']).cpu().numpy()
    if t['classic']:
        return [0.0 if a == -1 else float(a) for a in ap[:, 0]]     # classic protocol has no -1 (generic.py:199-208)
    return [{'easy': float(a[0]) if a[0] != -1 else -1, 'medium': float(a[1]) if a[1] != -1 else -1,
             'hard': float(a[2]) if a[2] != -1 else -1} for a in ap]


# ---- class-labelled datasets: ImageListLabels / ImageListLabelsQ ----------------------------------------------------
def build_label_tables(db):
    """Host-side tables for eval_labelled_device, built once per dataset from db.labels / db.c_relevant_idx and
    db.get_query_db() (dirtorch/datasets/dataset.py:70-101) - plain Python and numpy, no GPU:
        labels [N]          class id of every database image (classes numbered in order of first appearance)
        class_off [C+1], class_members [N]   CSR of the database indices of every class, shared by all its queries
        qclass [Q]          class id of the query's label, -1 when no database image carries it
        qself [Q]           the query's own database index when the queries ARE the database, else -1
    all int32 ndarrays; plus C and same_set."""
    query_db = db.get_query_db()
    same_set = query_db is db
    N = len(db.labels)
    cid = {label: c for c, label in enumerate(db.c_relevant_idx)}
    labels = np.fromiter((cid[l] for l in db.labels), dtype=np.int32, count=N)
    sizes = [len(db.c_relevant_idx[label]) for label in cid]
    class_off = np.zeros(len(cid) + 1, dtype=np.int32)
    class_off[1:] = np.cumsum(sizes)
    class_members = np.fromiter((i for label in cid for i in db.c_relevant_idx[label]), dtype=np.int32, count=N)
    Q = len(query_db)
    qclass = np.fromiter((cid.get(query_db.get_label(q), -1) for q in range(Q)), dtype=np.int32, count=Q)
    qself = np.arange(Q, dtype=np.int32) if same_set else -np.ones(Q, dtype=np.int32)
    return dict(labels=labels, class_off=class_off, class_members=class_members, qclass=qclass, qself=qself,
                C=len(cid), same_set=same_set)


def eval_labelled_device(db, qdescs, bdescs, tables=None, k=(1, 5, 10, 20, 50, 100), scratch_bytes=256 << 20):
    """(aps, tops) of a class-labelled dataset: the lists `[db.eval_query_AP(q, s) ...]` and `[db.eval_query_top(q, s, k)
    ...]` build from the rows s of the score matrix (dirtorch/test_dir.py:153-178) - floats with -1 for a query without
    positives, and one {k_: 0.0 / 1.0} dict per query over the k_ < N - without that matrix: the queries are scored
    (similarity_device's kernels) and ranked (ops.label_rank) in row chunks of scratch_bytes, each chunk dropped before
    the next, and 12 bytes per query come back.  Ties at a top-k boundary break by ascending index (a stable argsort).
    A chunk's scores are what ops.similarity gives for that block of queries: the fp32 GEMM starts every tile's sum at
    its own K slab (csrc/gemm_f32.hip), so against the whole-matrix call the last bits of a score can differ once K has
    more than two slabs of 32, and two near-equal neighbours can swap (one AP moved by 6.9e-5, the mAP by 3.3e-9, at Q = N = 20000, D = 2048 in six chunks).
    A row with a NaN or infinite kept score raises ValueError, as sklearn does on the host path."""
    from .utils.common import _dev
    t = tables if tables is not None else build_label_tables(db)
    q, b = _dev(qdescs), _dev(bdescs)
    Q, N = q.shape[0], b.shape[0]
    assert Q == len(t['qclass']) and N == len(t['labels']), "descriptors should have %d and %d rows" % (
        len(t['qclass']), len(t['labels']))
    if Q == 0:
        return [], []
    dev = {name: torch.as_tensor(t[name], dtype=torch.int32).to(b.device)
           for name in ('labels', 'class_off', 'class_members', 'qclass', 'qself')}
    # one verdict for every chunk (similarity_device's rule), so that a chunk's scores do not depend on the chunking
    owned = b is bdescs
    unit = bool(N >= UNIT_RANGE_MIN_ROWS and (database_is_unit_range(b) if owned else is_unit_range(b))
                and is_unit_range(q))
    rows = int(max(1, min(Q, scratch_bytes // max(4 * N, 1))))
    ap = torch.empty(Q, dtype=torch.float64, device=b.device)
    best = torch.empty(Q, dtype=torch.int32, device=b.device)
    for r0 in range(0, Q, rows):
        r1 = min(Q, r0 + rows)
        scores = ops.similarity(q[r0:r1], b, unit_range=unit)
        ap[r0:r1], best[r0:r1] = ops.label_rank(scores, dev['labels'], dev['class_off'], dev['class_members'],
                                                dev['qclass'][r0:r1], dev['qself'][r0:r1])
        del scores
    ap, best = ap.cpu().numpy(), best.cpu().numpy()
    bad = np.flatnonzero(np.isnan(ap))
    if len(bad):
        raise ValueError('query %d: its scores contain NaN or infinity' % int(bad[0]))
    aps = [-1 if a == -1 else float(a) for a in ap]
    tops = [{k_: float(r < k_) for k_ in k if k_ < N} for r in best.tolist()]
    return aps, tops


# ---- ranked neighbour lists -----------------------------------------------------------------------------------------
def retrieve_device(qdescs, bdescs, k, same_set=False, scratch_bytes=256 << 20, db_rows=None):
    """(idx [Q,k] int32, vals [Q,k] float32), both CUDA: the k best database rows of every query, best first, and their
    scores - np.argsort(scores[q], kind='stable')[::-1][:k] of the rows of qdescs . bdescs^T (ops.topk's order: larger
    index first among equal scores, NaN last) - without the Q x N matrix: the queries are scored (similarity_device's
    kernels) and ranked (ops.topk) in row chunks of scratch_bytes, each chunk dropped before the next -
    eval_labelled_device's loop, with its single unit-range verdict for all chunks.  1 <= k <= min(N, ops.topk_max_k()).
    same_set=True (the queries ARE the database): row q's own index is left out, and a list of k = N ends in (-1, NaN).
    db_rows: walk the database in blocks of that many rows as well; a block's k best are merged into the running list
    through ops.topk's id table (the list and the block's candidates, 2k columns), so the scratch holds rows x db_rows
    scores.  Lists of database shards merge the same way: concatenate (vals, idx + shard offset) and call ops.topk with
    ids.  The lists depend on the scores alone; a score's last bits can depend on the chunking (eval_labelled_device)."""
    from .utils.common import _dev
    q, b = _dev(qdescs), _dev(bdescs)
    Q, N = q.shape[0], b.shape[0]
    k = int(k)
    if k < 1 or k > min(N, ops.topk_max_k()):
        raise ValueError('1 <= k <= min(N, %d) expected, got k = %d for N = %d' % (ops.topk_max_k(), k, N))
    if same_set and Q != N:
        raise ValueError('same_set: the queries are the database, got %d and %d rows' % (Q, N))
    block = N if db_rows is None else int(max(k, min(N, db_rows)))     # (a block offers k candidates: at least k rows)
    idx = torch.empty(Q, k, dtype=torch.int32, device=b.device)
    vals = torch.empty(Q, k, dtype=torch.float32, device=b.device)
    if Q == 0:
        return idx, vals
    owned = b is bdescs
    unit = bool(N >= UNIT_RANGE_MIN_ROWS and (database_is_unit_range(b) if owned else is_unit_range(b))
                and is_unit_range(q))
    rows = int(max(1, min(Q, scratch_bytes // max(4 * block, 1))))
    for r0 in range(0, Q, rows):
        r1 = min(Q, r0 + rows)
        own = torch.arange(r0, r1, dtype=torch.int32, device=b.device) if same_set else None
        run_i = run_v = None
        for b0 in range(0, N, block):
            b1 = min(N, b0 + block)
            scores = ops.similarity(q[r0:r1], b[b0:b1], unit_range=unit)
            if b0 == 0 and b1 == N:
                run_i, run_v = ops.topk(scores, k, exclude=own)
                break
            kb = min(k, b1 - b0)                                   # (only a ragged last block is shorter than k)
            bi, bv = ops.topk(scores, kb, exclude=None if own is None else own - b0)
            del scores
            bi = torch.where(bi >= 0, bi + b0, bi)                 # block columns -> database rows; -1 stays a hole
            if run_i is None:                                      # (the first block has at least k rows)
                run_i, run_v = bi, bv
            else:
                run_i, run_v = ops.topk(torch.cat([run_v, bv], dim=1), k, ids=torch.cat([run_i, bi], dim=1))
        idx[r0:r1], vals[r0:r1] = run_i, run_v
    return idx, vals


# ---- alpha query expansion / database augmentation from neighbour lists --------------------------------------------------
def expand_device(descs, db=None, alpha=0, k=0, index=None, scratch_bytes=256 << 20, **search_kw):
    """test_dir.expand_descriptors (dirtorch/test_dir.py:24-44) from neighbour LISTS -> CUDA fp32 [n, D]:
    out[i] = normalize(mean(descs[i], score^alpha * db[j] for the k neighbours j of descs[i])), without the n x m score
    matrix of the matrix route (ops.expand_descriptors): the lists are made first, then ops.expand_lists gathers k + 1 rows
    per output row (include/dir_engine.h gives the arithmetic, tests/expand_ref.py restates it).
    db=None: the set is expanded against itself (DBA) and a row is not its own neighbour (same_set lists).  k == 0 returns
    `descs` itself, the reference's contract; a negative k or alpha raises ValueError.
    index=None: exact lists, retrieve_device(descs, db, k, same_set=...).  Otherwise `index` is one of the four classes of
    dirtorch_amd.index and already holds exactly the rows of db (of descs for the self-set) - len(index) and index.D are
    checked, the contents are the caller's word - and the lists are index.search(descs, k, same_set=..., **search_kw);
    search_kw carries nprobe, rerank and source (source defaults to the rows themselves when rerank is given).  With rerank
    the weights are fp32 scores; without it they are the index's quantised or table scores, and an inverted file probed
    too narrowly gives lists that end in empty slots, which add nothing (the mean still divides by k + 1).
    1 <= k <= min(m, ops.topk_max_k()) is inherited from the list makers; the matrix route keeps its "any k".
    The one semantic difference from the matrix route: the reference zeroes the diagonal of a self-set, so a row can still
    pick ITSELF, with weight 0^alpha, when fewer than k other rows score above 0; the list route never picks the row
    itself and takes the k best other rows whatever their sign."""
    from .utils.common import _dev
    k = int(k)
    if k < 0 or alpha < 0:
        raise ValueError('k and alpha must be non-negative, got k = %d, alpha = %g' % (k, alpha))
    if k == 0:
        return descs
    same_set = db is None
    x = _dev(descs)
    pool_ = x if same_set else _dev(db)
    if x.dim() != 2 or pool_.dim() != 2 or x.shape[1] != pool_.shape[1]:
        raise ValueError('descs [n, D] and db [m, D] expected')
    if index is None:
        if search_kw:
            raise TypeError('%s only apply to an index' % ', '.join(sorted(search_kw)))
        idx, vals = retrieve_device(x, pool_, k, same_set=same_set, scratch_bytes=scratch_bytes)
    else:
        if len(index) != pool_.shape[0] or index.D != pool_.shape[1]:
            raise ValueError('an index over the %d x %d rows of db expected, got %d x %d' % (
                pool_.shape[0], pool_.shape[1], len(index), index.D))
        if search_kw.get('rerank') and search_kw.get('source') is None:
            search_kw = dict(search_kw, source=pool_)
        idx, vals = index.search(x, k, same_set=same_set, scratch_bytes=scratch_bytes, **search_kw)
    return ops.expand_lists(x, pool_, idx, vals, float(alpha))


# ---- diffusion re-ranking on the database's kNN graph -------------------------------------------------------------------
def _lists(x, pool_, k, same_set, index, scratch_bytes, search_kw):
    """neighbour lists of x among pool_: exact (retrieve_device) or from an index over pool_, with expand_device's checks"""
    if index is None:
        if search_kw:
            raise TypeError('%s only apply to an index' % ', '.join(sorted(search_kw)))
        return retrieve_device(x, pool_, k, same_set=same_set, scratch_bytes=scratch_bytes)
    if len(index) != pool_.shape[0] or index.D != pool_.shape[1]:
        raise ValueError('an index over the %d x %d rows of the database expected, got %d x %d' % (
            pool_.shape[0], pool_.shape[1], len(index), index.D))
    if search_kw.get('rerank') and search_kw.get('source') is None:
        search_kw = dict(search_kw, source=pool_)
    return index.search(x, k, same_set=same_set, scratch_bytes=scratch_bytes, **search_kw)


def knn_graph_device(bdescs, k, gamma=3, index=None, scratch_bytes=256 << 20, **search_kw):
    """(idx [N,k] int32, S [N,k] fp32), both CUDA: the mutual kNN graph of the database, normalised (ops.knn_graph;
    include/dir_engine.h gives the arithmetic) - the offline stage of diffuse_device, reusable across query sets.
    The k neighbours of every row are retrieve_device(bdescs, bdescs, k, same_set=True), or with `index` (one of the four
    classes of dirtorch_amd.index, already holding exactly the rows of bdescs) index.search(bdescs, k, same_set=True,
    **search_kw); search_kw carries nprobe, rerank and source (source defaults to the rows themselves when rerank is
    given).  Lists that end in empty slots, as a narrowly probed inverted file gives, only make the graph sparser."""
    from .utils.common import _dev
    b = _dev(bdescs)
    if b.dim() != 2:
        raise ValueError('bdescs [N, D] expected')
    idx, vals = _lists(b, b, int(k), True, index, scratch_bytes, search_kw)
    return idx, ops.knn_graph(idx, vals, gamma)


def diffuse_device(qdescs, bdescs, k=50, kq=10, gamma=3, alpha=0.99, iters=20, graph=None, index=None,
                   scratch_bytes=256 << 20, **search_kw):
    """Diffusion scores [Q, N] fp32 CUDA, contiguous - the "+DFS" row of the revisited Oxford / Paris tables (Iscen et al.,
    "Efficient Diffusion on Region Manifolds", global descriptors): the kq best database rows of every query seed a
    column (score^gamma), and (I - alpha S) f = y is solved on the mutual k-NN graph S of the database by `iters`
    conjugate-gradient iterations on the device (ops.diffusion_seed, ops.diffusion_solve).  The result fits ops.topk,
    ops.rank_counts and eval_aps_device unchanged.  graph: (idx, S) of knn_graph_device(bdescs, k, gamma, ...), made once
    per database; None: it is made here.  index / search_kw: as in knn_graph_device, for the graph (when made here) and
    for the queries' lists.
    The queries are a set of their own: a query that is a database row would need a one-hot seed at its own row and that
    row kept out of its list, which this does not do - passing the database as the query set raises ValueError."""
    from .utils.common import _dev
    q, b = _dev(qdescs), _dev(bdescs)
    if q.dim() != 2 or b.dim() != 2 or q.shape[1] != b.shape[1]:
        raise ValueError('qdescs [Q, D] and bdescs [N, D] expected')
    if qdescs is bdescs or (q.data_ptr() == b.data_ptr() and q.shape == b.shape):
        raise ValueError('diffuse_device: the query set is the database itself - queries that are database rows are not '
                         'supported (the queries must be a set of their own)')
    N = b.shape[0]
    if graph is None:
        graph = knn_graph_device(b, k, gamma, index=index, scratch_bytes=scratch_bytes, **search_kw)
    idx, S = graph
    if idx.shape[0] != N or tuple(S.shape) != tuple(idx.shape):
        raise ValueError('a graph (idx, S) over the %d rows of the database expected' % N)
    qidx, qvals = _lists(q, b, int(kq), False, index, scratch_bytes, search_kw)
    Y = ops.diffusion_seed(qidx, qvals, N, gamma)
    F = ops.diffusion_solve(idx, S, Y, alpha=alpha, iters=iters)
    return F.t().contiguous()


def diffuse_truncated_device(qdescs, bdescs, trunc=1000, k=50, kq=10, gamma=3, alpha=0.99, iters=20, graph=None, index=None,
                             same_set=False, dense=False, scratch_bytes=256 << 20, **search_kw):
    """Truncated diffusion: every query solved on the subgraph of its `trunc` best database rows, as Iscen et al. do at
    query time - (idx [Q, trunc] int32, vals [Q, trunc] fp32), both CUDA: the candidates re-ranked by their diffusion
    score, best first (ops.topk over the list scores with the candidates' ids; dead candidates end as (-1, NaN)).
    The candidates are the `trunc` best rows of every query - exact (retrieve_device) or index.search(..., **search_kw) -
    with trunc clipped to N and at most ops.diffusion_local_max_rows(); the first kq of them seed the solve (score^gamma).
    The subgraph of the candidates is cut out of the graph (ops.diffusion_subgraph) and (I - alpha S_q) f = y_q is solved
    by `iters` conjugate-gradient iterations in one workgroup per query and one launch (ops.diffusion_solve_local):
    nothing of size N is touched after the lists.  graph / index / search_kw: as in diffuse_device.
    same_set=True: the queries ARE the database rows (qdescs and bdescs hold the same rows): the query's own row is
    candidate 0 with a one-hot seed, followed by its trunc - 1 best other rows - the case diffuse_device refuses.
    dense=True: scores [Q, N] fp32 CUDA instead, for eval_aps_device, ops.topk and ops.rank_counts: the similarities
    (similarity_device) minus 4, a candidate's column overwritten by max(f, -2) (ops.diffusion_spread), so every candidate
    outranks every other row and the other rows keep their cosine order."""
    from .utils.common import _dev
    q, b = _dev(qdescs), _dev(bdescs)
    if q.dim() != 2 or b.dim() != 2 or q.shape[1] != b.shape[1]:
        raise ValueError('qdescs [Q, D] and bdescs [N, D] expected')
    Q, N = q.shape[0], b.shape[0]
    if same_set and Q != N:
        raise ValueError('same_set: the queries are the database, got %d and %d rows' % (Q, N))
    trunc = min(int(trunc), N)
    if trunc < (2 if same_set else 1) or trunc > ops.diffusion_local_max_rows():
        raise ValueError('%d <= trunc <= %d expected, got %d (N = %d)' % (2 if same_set else 1, ops.diffusion_local_max_rows(),
                                                                          trunc, N))
    if graph is None:
        graph = knn_graph_device(b, k, gamma, index=index, scratch_bytes=scratch_bytes, **search_kw)
    idx, S = graph
    if idx.shape[0] != N or tuple(S.shape) != tuple(idx.shape):
        raise ValueError('a graph (idx, S) over the %d rows of the database expected' % N)
    if same_set:
        oidx, ovals = _lists(q, b, trunc - 1, True, index, scratch_bytes, search_kw)
        own = torch.arange(Q, dtype=torch.int32, device=b.device)[:, None]
        cidx = torch.cat([own, oidx], dim=1)
        cvals = torch.cat([torch.ones(Q, 1, dtype=torch.float32, device=b.device), ovals], dim=1)
    else:
        cidx, cvals = _lists(q, b, trunc, False, index, scratch_bytes, search_kw)
    cid, lidx, lw, y = ops.diffusion_subgraph(idx, S, cidx, cvals, kq=int(kq), gamma=gamma, one_hot=same_set)
    f = ops.diffusion_solve_local(lidx, lw, y, cid=cid, alpha=alpha, iters=iters)
    if not dense:
        if Q == 0:
            return cid, f
        return ops.topk(f, trunc, ids=cid)
    return ops.diffusion_spread(similarity_device(q, b), cid, f)      # (a fresh matrix: changed in place)

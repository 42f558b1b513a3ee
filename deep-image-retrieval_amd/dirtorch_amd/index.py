"""The int8 descriptor index: a database kept as per-row int8 codes with one fp32 scale per row (a quarter of the fp32
bytes), scanned on the int8 matrix cores and, on request, re-ranked with the full-precision rows.

    index = Int8Index(D)
    index.add(bdescs)                                        # CUDA / CPU tensor, ndarray or memmap: quantised in row chunks
    idx, vals = index.search(qdescs, 10)                     # lists by quantised score
    idx, vals = index.search(qdescs, 10, rerank=40, source=bdescs)   # shortlist of 40, re-scored in fp32, then the 10 best

include/dir_engine.h defines the quantisation and the quantised score; an int8 dot product accumulated in int32 is exact,
so a quantised score is one defined fp32 number and the lists of a scan do not depend on scratch_bytes, db_rows or on how
many add() calls built the database.

The fp4 index halves the row again - 4-bit block-scaled codes (D <= ops.index_fp4_max_dim()) on the scaled matrix cores:

    index = Fp4Index(D)
    index.add(bdescs)
    idx, vals = index.search(qdescs, 10, rerank=40, source=bdescs)   # its raw scores are coarse: made for use with rerank

Every partial sum of one of its scores is exact in fp32 (include/dir_engine.h), so its lists are those of tests/fp4_ref.py bit
for bit and as independent of the cut of the work as Int8Index's.

The binary index keeps one sign bit per value and one fp32 scale per row - 260 bytes a row of 2048, a quarter of the fp4 row -
and scores int8-coded queries against them on the int8 matrix cores:

    index = BinaryIndex(D)
    index.add(bdescs)
    idx, vals = index.search(qdescs, 10, rerank=1280, source=bdescs)   # its raw lists are coarser still: use a long shortlist

Its sum is an exact int32, so its lists are those of tests/bin_ref.py bit for bit and as independent of the cut of the work.

The inverted file reads only the lists a query falls into instead of the whole database:

    index = IVFInt8Index(D, nlist=1024)
    index.train(bdescs)                                      # spherical k-means on (a sample of) the descriptors
    index.add(bdescs)                                        # quantised, assigned to a list, stored list-major
    idx, vals = index.search(qdescs, 10, nprobe=8)           # the 8 best lists of every query are scanned
    idx, vals = index.search(qdescs, 10, nprobe=8, rerank=40, source=bdescs)

Its assignment, probing and scores are defined through the quantised score as well (include/dir_engine.h), so with
nprobe = nlist it returns Int8Index's lists bit for bit, and with fewer lists those of tests/ivf_ref.py.

The inverted file over fp4 codes keeps Fp4Index's rows in IVFInt8Index's lists - the same coarse quantiser (a row lands in
the same list), 1096 bytes a row of 2048 instead of 2056:

    index = IVFFp4Index(D, nlist=1024)                       # D <= ops.index_fp4_max_dim()
    index.train(bdescs)                                      # IVFInt8Index.train
    index.add(bdescs)
    idx, vals = index.search(qdescs, 10, nprobe=8, rerank=40, source=bdescs)   # coarse raw scores: made for use with rerank

Its scores are Fp4Index's numbers, so with nprobe = nlist it returns Fp4Index's lists bit for bit, and with fewer lists those
of tests/ivffp4_ref.py.

The inverted file over sign-bit rows keeps BinaryIndex's rows in the same lists, 264 bytes a row of 2048:

    index = IVFBinaryIndex(D, nlist=1024)                    # D <= ops.index_bin_max_dim()
    index.train(bdescs)                                      # IVFInt8Index.train
    index.add(bdescs)
    idx, vals = index.search(qdescs, 10, nprobe=8, rerank=2048, source=bdescs)   # coarse raw lists: use a long shortlist

Its scores are BinaryIndex's numbers, so with nprobe = nlist it returns BinaryIndex's lists bit for bit, and with fewer
lists those of tests/ivfbin_ref.py.

The product-quantised index keeps M bytes per row instead of D - a row is the numbers of its nearest of 256 centroids in
each of M sub-spaces - and scores a query through M tables of 256 inner products:

    index = PQIndex(D, M)                                    # M divides D, 1 <= M <= ops.pq_max_m()
    index.train(bdescs)                                      # Lloyd iterations per sub-space on (a sample of) the descriptors
    index.add(bdescs)                                        # encoded in row chunks
    idx, vals = index.search(qdescs, 10)                     # lists by table score
    idx, vals = index.search(qdescs, 10, rerank=40, source=bdescs)

Codes, tables and scores are chains of single fp32 operations in a fixed order (include/dir_engine.h): the lists are those
of tests/pq_ref.py bit for bit and do not depend on scratch_bytes, db_rows or on how many add() calls built the database.

IVF-PQ puts the two together: the inverted file's lists hold M-byte codes of the RESIDUAL of a row to the centroid of its
list, and a query reads the codes of its probed lists only:

    index = IVFPQIndex(D, nlist=1024, M=64)
    index.train(bdescs)                                      # the inverted file's k-means, then PQ codebooks on the residuals
    index.add(bdescs)                                        # assigned as IVFInt8Index does, residuals encoded, stored list-major
    idx, vals = index.search(qdescs, 10, nprobe=8)
    idx, vals = index.search(qdescs, 10, nprobe=8, rerank=40, source=bdescs)

A row lands in the list IVFInt8Index puts it in; the score is the coarse term <q, centroid> plus the row's table entries,
one chain of fp32 additions (include/dir_engine.h), and the lists are those of tests/ivfpq_ref.py bit for bit.
"""
import numpy as np
import torch

from . import ops
from .utils.common import _dev

ADD_CHUNK_BYTES = 256 << 20     # fp32 bytes of a database that are on the device at a time while it is quantised
DEFAULT_PLAN = 'auto'           # search(plan=) of the inverted files: the device plan was the faster one at every measured
                                # point (profiles/ivf_plan.txt: 0.44 - 0.72 of the host plan's time)


def _round_up(n, to):
    return (n + to - 1) // to * to


def _is_host(x):
    return isinstance(x, np.ndarray) or (torch.is_tensor(x) and not x.is_cuda)


def _upload(x):
    """rows of an ndarray / memmap / tensor -> contiguous fp32 CUDA tensor"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device='cuda', dtype=torch.float32).contiguous()


def _row_chunks(descs, D):
    """The rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap) as contiguous fp32 CUDA tensors, one chunk
    of ADD_CHUNK_BYTES at a time, so a database that lives in a host file is never resident on the device as fp32."""
    rows = max(1, ADD_CHUNK_BYTES // (4 * D))
    for r0 in range(0, int(descs.shape[0]), rows):
        yield _upload(descs[r0:r0 + rows])


def _appended(stores, descs, D, encode):
    """The flat stores [N, ...] of an index, each grown by the rows of descs [n, D]: copied once, then filled chunk by
    chunk with encode(x) -> one tensor per store for the rows of the chunk x."""
    n, r0 = int(descs.shape[0]), len(stores[0])
    out = [torch.empty((r0 + n,) + tuple(s.shape[1:]), dtype=s.dtype, device='cuda') for s in stores]
    for o, s in zip(out, stores):
        o[:r0] = s
    for x in _row_chunks(descs, D):
        for o, part in zip(out, encode(x)):
            o[r0:r0 + len(x)] = part
        r0 += len(x)
    return out


def _training_rows(x, seed, max_rows, least, least_name):
    """The training sample of a train() call as a contiguous fp32 CUDA tensor: the rows of x, or the sorted
    np.random.RandomState(seed).choice sample of max_rows of them when x has more; at least `least` finite rows."""
    n = int(x.shape[0])
    if n < least or max_rows < least:
        raise ValueError('at least %s training rows expected, got %d' % (least_name, min(n, max_rows)))
    if n > max_rows:
        pick = np.sort(np.random.RandomState(seed).choice(n, max_rows, replace=False))
        x = x[torch.from_numpy(pick).to(x.device)] if torch.is_tensor(x) else x[pick]
    x = _upload(x)
    if not bool(torch.isfinite(x).all()):
        raise ValueError('training data with a non-finite value')
    return x


def _segment_sums(x, assign, bounds):
    """The step the two Lloyd loops share.  assign [n]: the segment of every row of x [n, d]; bounds: arange(S + 1) on the
    device.  -> (seg_off [S+1] int32, sums [S, d] fp32): a stable sort of the assignment, so a segment adds its rows up in
    ascending row order (ops.segment_sums); an empty segment has seg_off[s] == seg_off[s+1] and sums to zero."""
    key, order = torch.sort(assign.long(), stable=True)
    seg_off = torch.searchsorted(key, bounds).to(torch.int32)
    return seg_off, ops.segment_sums(x, order.to(torch.int32), seg_off)


def _read_npz(path):
    with np.load(path) as f:
        return {name: f[name] for name in f.files}


def _padded_codes(path, codes, width, dtype, pitch):
    """a saved code matrix [N, width] -> the device store [N, width rounded up to pitch], the padding zero"""
    if codes.dtype != dtype or codes.ndim != 2 or codes.shape[1] != width:
        raise ValueError('%s: codes [N, %d] %s expected' % (path, width, np.dtype(dtype).name))
    codes = torch.from_numpy(codes).cuda()
    store = torch.zeros(len(codes), _round_up(width, pitch), dtype=codes.dtype, device='cuda')
    store[:, :width] = codes
    return store


def _scales_of(path, f, N, rows):
    """the saved `scales` of N rows -> fp32 CUDA; rows: how the message names what they belong to"""
    if f['scales'].shape != (N,):
        raise ValueError('%s: scales [N] expected for %s' % (path, rows))
    return torch.from_numpy(f['scales'].astype(np.float32)).cuda()


class _Int8Store:
    """The code store of a format, once per format: `names`, the per-row CUDA tensors an index keeps (in the order its
    quantiser returns and its scorer takes them), max_dim() the widest row, empty(D) -> those tensors with no rows,
    quantize(x) -> those of the rows of a chunk, save(index) -> the store's arrays of a .npz, load(path, f, D) -> the tensors
    from such arrays.  Here the int8 one: codes [N, D rounded up to 64] int8 (padding zero), scales [N] fp32."""
    names = ('codes', 'scales')
    max_dim = staticmethod(ops.index_i8_max_dim)
    quantize = staticmethod(ops.quantize_rows)

    @staticmethod
    def empty(D):
        return (torch.empty(0, _round_up(D, 64), dtype=torch.int8, device='cuda'),
                torch.empty(0, dtype=torch.float32, device='cuda'))

    @staticmethod
    def save(index):
        """`codes` [N, D] int8 (without the padding), `scales` [N] float32"""
        return dict(codes=index.codes[:, :index.D].cpu().numpy(), scales=index.scales.cpu().numpy())

    @staticmethod
    def load(path, f, D):
        codes = _padded_codes(path, f['codes'], D, np.int8, 64)
        return codes, _scales_of(path, f, len(codes), 'codes [N, D]')


class _Fp4Store:
    """The fp4 store: codes [N, ldc] uint8, exps [N, lde] uint8, scales [N] fp32; (ldc, lde) = ops.fp4_widths(D)."""
    names = ('codes', 'exps', 'scales')
    max_dim = staticmethod(ops.index_fp4_max_dim)
    quantize = staticmethod(ops.quantize_rows_fp4)

    @staticmethod
    def empty(D):
        ldc, lde = ops.fp4_widths(D)
        return (torch.empty(0, ldc, dtype=torch.uint8, device='cuda'), torch.empty(0, lde, dtype=torch.uint8, device='cuda'),
                torch.empty(0, dtype=torch.float32, device='cuda'))

    @staticmethod
    def save(index):
        """`codes` [N, ceil(D / 2)] uint8, `exps` [N, ceil(D / 32)] uint8 (both without the padding), `scales` [N] float32"""
        nc, ne = (index.D + 1) // 2, (index.D + 31) // 32
        return dict(codes=index.codes[:, :nc].cpu().numpy(), exps=index.exps[:, :ne].cpu().numpy(),
                    scales=index.scales.cpu().numpy())

    @staticmethod
    def load(path, f, D):
        ldc, lde = ops.fp4_widths(D)
        codes = _padded_codes(path, f['codes'], (D + 1) // 2, np.uint8, ldc)
        N, ne = len(codes), (D + 31) // 32
        if f['exps'].dtype != np.uint8 or f['exps'].shape != (N, ne):
            raise ValueError('%s: exps [N, %d] uint8 expected for codes of N rows' % (path, ne))
        exps = torch.full((N, lde), 127, dtype=torch.uint8, device='cuda')
        exps[:, :ne] = torch.from_numpy(f['exps']).cuda()
        return codes, exps, _scales_of(path, f, N, 'codes [N, ...]')


class _BinStore:
    """The sign-bit store: the bits as codes [N, ops.bin_width(D)] uint8 (padding zero), scales [N] fp32."""
    names = ('codes', 'scales')
    max_dim = staticmethod(ops.index_bin_max_dim)
    quantize = staticmethod(ops.quantize_rows_bin)

    @staticmethod
    def empty(D):
        return (torch.empty(0, ops.bin_width(D), dtype=torch.uint8, device='cuda'),
                torch.empty(0, dtype=torch.float32, device='cuda'))

    @staticmethod
    def save(index):
        """`bits` [N, ceil(D / 8)] uint8 (without the padding), `scales` [N] float32"""
        return dict(bits=index.codes[:, :(index.D + 7) // 8].cpu().numpy(), scales=index.scales.cpu().numpy())

    @staticmethod
    def load(path, f, D):
        codes = _padded_codes(path, f['bits'], (D + 7) // 8, np.uint8, 16)
        return codes, _scales_of(path, f, len(codes), 'bits [N, ...]')


class _CodedIndex:
    """What every index shares: a code store (`_store`: one of the classes above, the int8 one unless a class says otherwise)
    whose tensors - `codes` [N, ldc], one row per database row, and what the format keeps beside it - are attributes of the
    index, made empty by the constructor, with the store's half of save and load (_save_store, _load_store); the
    product-quantised indexes replace codes by uint8 ones with ldc = M rounded up to 4 and scales by None - what a search
    does around its scan (the argument checks, the fp32 re-rank of a shortlist) and the blocked scan loop."""

    _store = _Int8Store

    def __init__(self, D):
        D = int(D)
        if D < 1 or D > self._store.max_dim():
            raise ValueError('1 <= D <= %d expected, got %d' % (self._store.max_dim(), D))
        self.D = D
        self._set_store(self._store.empty(D))

    def _stored(self):
        """the store's tensors, in the order of its names"""
        return [getattr(self, name) for name in self._store.names]

    def _set_store(self, tensors):
        for name, t in zip(self._store.names, tensors):
            setattr(self, name, t)

    def _load_store(self, path, f):
        self._set_store(self._store.load(path, f, self.D))

    def __len__(self):
        return int(self.codes.shape[0])

    def _trained(self):
        """whether add, search and save have what they need (the mixins below add their conditions)"""
        return True

    def _need_trained(self, what):
        if not self._trained():
            raise ValueError('%s before train' % what)

    def _check_rows(self, descs):
        if descs.ndim != 2 or descs.shape[1] != self.D:
            raise ValueError('descriptors [n, %d] expected' % self.D)

    def _check_train(self, x):
        self._check_rows(x)
        if len(self):
            raise ValueError('train before add: the rows already stored were coded with the old centroids / codebooks')

    def _search(self, qdescs, k, rerank, source, same_set, scratch_bytes, scan):
        """What every search does around its scan: the queries to the device, the argument checks, the empty result of an
        empty query set, scan(q, keep) -> the (cand, vals) [Q, keep] of the keep = rerank or k best rows of every query,
        and - with rerank - the k best of those by fp32 score against `source`."""
        self._need_trained('search')
        q = _dev(qdescs)
        k, R = int(k), int(rerank)
        Q, N = q.shape[0], len(self)
        if q.dim() != 2 or q.shape[1] != self.D:
            raise ValueError('queries [Q, %d] expected' % self.D)
        kmax = min(N, ops.topk_max_k())
        if k < 1 or k > kmax:
            raise ValueError('1 <= k <= min(N, %d) expected, got k = %d for N = %d' % (ops.topk_max_k(), k, N))
        if R and (R < k or R > kmax):
            raise ValueError('k <= rerank <= min(N, %d) expected, got rerank = %d for k = %d, N = %d' % (
                ops.topk_max_k(), R, k, N))
        if R and source is None:
            raise ValueError('rerank needs the fp32 database as `source`')
        if R and (source.ndim != 2 or tuple(source.shape) != (N, self.D)):
            raise ValueError('source [%d, %d] expected' % (N, self.D))
        if same_set and Q != N:
            raise ValueError('same_set: the queries are the database, got %d and %d rows' % (Q, N))
        if Q == 0:
            return (torch.empty(0, k, dtype=torch.int32, device='cuda'),
                    torch.empty(0, k, dtype=torch.float32, device='cuda'))
        cand, vals = scan(q, R or k)
        if not R:
            return cand, vals
        return ops.topk(self._rescore(q, cand, source, scratch_bytes), k, ids=cand)

    def _scan_blocks(self, Q, keep, same_set, scratch_bytes, db_rows, scorer, row_bytes=0):
        """ranking.retrieve_device's loop on a coded database: the `keep` best rows of every query.  scorer(r0, r1) -> a
        function (b0, b1) -> the scores [r1 - r0, b1 - b0] of queries r0 .. r1 against rows b0 .. b1.  The queries go in
        chunks whose score rows (and row_bytes more per query: what a scorer holds for its chunk) fit scratch_bytes."""
        N = len(self)
        block = N if db_rows is None else int(max(keep, min(N, db_rows)))
        idx = torch.empty(Q, keep, dtype=torch.int32, device='cuda')
        vals = torch.empty(Q, keep, dtype=torch.float32, device='cuda')
        rows = int(max(1, min(Q, scratch_bytes // max(4 * block + row_bytes, 1))))
        for r0 in range(0, Q, rows):
            r1 = min(Q, r0 + rows)
            own = torch.arange(r0, r1, dtype=torch.int32, device='cuda') if same_set else None
            score = scorer(r0, r1)
            run_i = run_v = None
            for b0 in range(0, N, block):
                b1 = min(N, b0 + block)
                scores = score(b0, b1)
                if b0 == 0 and b1 == N:
                    run_i, run_v = ops.topk(scores, keep, exclude=own)
                    break
                kb = min(keep, b1 - b0)
                bi, bv = ops.topk(scores, kb, exclude=None if own is None else own - b0)
                del scores
                bi = torch.where(bi >= 0, bi + b0, bi)
                if run_i is None:
                    run_i, run_v = bi, bv
                else:
                    run_i, run_v = ops.topk(torch.cat([run_v, bv], dim=1), keep, ids=torch.cat([run_i, bi], dim=1))
            idx[r0:r1], vals[r0:r1] = run_i, run_v
        return idx, vals

    def _rescore(self, q, cand, source, scratch_bytes):
        """fp32 scores [Q, R] of the candidates against the rows of source"""
        if not _is_host(source):
            return ops.gather_scores(q, source.to(dtype=torch.float32), cand)
        if torch.is_tensor(source):
            source = source.numpy()
        Q, R = cand.shape
        out = torch.empty(Q, R, dtype=torch.float32, device='cuda')
        rows = int(max(1, min(Q, scratch_bytes // max(4 * R * self.D, 1))))
        for r0 in range(0, Q, rows):
            r1 = min(Q, r0 + rows)
            c = cand[r0:r1].cpu().numpy()
            used = np.unique(c[c >= 0])                                   # sorted: one pass over a memmap
            picked = _upload(source[used]) if len(used) else torch.zeros(1, self.D, device='cuda')
            local = np.where(c >= 0, np.searchsorted(used, c), -1).astype(np.int32)
            out[r0:r1] = ops.gather_scores(q[r0:r1], picked, torch.from_numpy(local).cuda())
        return out


class _FlatIndex(_CodedIndex):
    """add, search, save, load and nbytes of the flat coded indexes.  A class states its `_store`, `_code_queries` (fp32
    queries -> the coded tensors of its scorer) and `_score(coded, r0, r1, b0, b1)`: the scores of the coded queries r0 .. r1
    against the stored rows b0 .. b1, one ops.similarity_* call written out flat (it runs once per block of every search)."""

    def nbytes(self):
        """the bytes the database rows take on the device: the store's tensors"""
        return sum(int(t.numel()) * t.element_size() for t in self._stored())

    def add(self, descs):
        """Append the rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap).  They are quantised in
        chunks of ADD_CHUNK_BYTES, so a database that lives in a host file is never resident on the device as fp32."""
        self._check_rows(descs)
        if int(descs.shape[0]):
            self._set_store(_appended(self._stored(), descs, self.D, self._store.quantize))
        return self

    def search(self, qdescs, k, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, db_rows=None):
        """(idx [Q,k] int32, vals [Q,k] float32), both CUDA, under ranking.retrieve_device's contract (its order, same_set
        leaving a query out of its own list, (-1, NaN) where a row runs short).  rerank = 0: ranked by the quantised
        scores, which vals carries.  rerank = R, k <= R <= min(N, ops.topk_max_k()): the scan keeps the R best per query,
        they are re-scored against `source` - the fp32 database: a CUDA tensor is gathered on the device, a host array
        or memmap has the candidates' rows gathered on the host in chunks of scratch_bytes - and vals carries the fp32
        scores of the k best of them."""
        def scan(q, keep):
            coded = self._code_queries(q)

            def scorer(r0, r1):
                return lambda b0, b1: self._score(coded, r0, r1, b0, b1)
            return self._scan_blocks(q.shape[0], keep, same_set, scratch_bytes, db_rows, scorer)
        return self._search(qdescs, k, rerank, source, same_set, scratch_bytes, scan)

    def save(self, path):
        """One .npz: the store's arrays (its save gives them) and `D`."""
        np.savez(path, D=np.int64(self.D), **self._store.save(self))

    @classmethod
    def load(cls, path):
        f = _read_npz(path)
        index = cls(int(f['D']))
        index._load_store(path, f)
        return index


class Int8Index(_FlatIndex):
    """codes [N, ldc] int8 (ldc = D rounded up to 64, padding zero) and scales [N] fp32, both CUDA.  save: one .npz of
    `codes` [N, D] int8 (without the padding), `scales` [N] float32, `D`."""
    _code_queries = staticmethod(ops.quantize_rows)

    def _score(self, coded, r0, r1, b0, b1):
        qc, qs = coded
        return ops.similarity_i8(qc[r0:r1], qs[r0:r1], self.codes[b0:b1], self.scales[b0:b1], self.D)


class Fp4Index(_FlatIndex):
    """The fp4 index (include/dir_engine.h gives the definition; numpy restatement: tests/fp4_ref.py): half of Int8Index's
    bytes.  codes [N, ldc] uint8 (two e2m1 values per byte), exps [N, lde] uint8 (one e8m0 byte per block of 32 values) and
    scales [N] fp32, all CUDA; (ldc, lde) = ops.fp4_widths(D).  A score is the exact inner product of the two dequantised
    rows, so the lists do not depend on how the scan or the adds were cut.  save: one .npz of `codes` [N, ceil(D / 2)]
    uint8, `exps` [N, ceil(D / 32)] uint8 (both without the padding), `scales` [N] float32, `D`."""
    _store = _Fp4Store
    _code_queries = staticmethod(ops.quantize_rows_fp4)

    def _score(self, coded, r0, r1, b0, b1):
        qc, qe, qs = coded
        return ops.similarity_fp4(qc[r0:r1], qe[r0:r1], qs[r0:r1], self.codes[b0:b1], self.exps[b0:b1], self.scales[b0:b1], self.D)


class BinaryIndex(_FlatIndex):
    """The binary index (include/dir_engine.h gives the definition; numpy restatement: tests/bin_ref.py): one sign bit
    per value and one fp32 scale per row, a quarter of Fp4Index's bytes.  codes [N, ldb] uint8 (ldb = ops.bin_width(D),
    bit k & 7 of byte k >> 3, padding zero) and scales [N] fp32, both CUDA.  The queries are coded as Int8Index codes
    them, and a score is ((float)t * qscale) * scale with t an exact int32, so the lists do not depend on how the scan
    or the adds were cut.  Its raw lists are coarse: pair it with rerank.  save: one .npz of `bits` [N, ceil(D / 8)] uint8
    (without the padding), `scales` [N] float32, `D`."""
    _store = _BinStore
    _code_queries = staticmethod(ops.quantize_rows)

    def _score(self, coded, r0, r1, b0, b1):
        qc, qs = coded
        return ops.similarity_bin(qc[r0:r1], qs[r0:r1], self.codes[b0:b1], self.scales[b0:b1], self.D)


class _InvertedLists:
    """What the inverted files share - the coarse quantiser and the list-major bookkeeping: centroids [nlist, D] fp32
    with their codes `ccodes` and scales `cscales`, ids [N] int32, list_off [nlist+1] int32 and `_lens`, the host copy of
    the list lengths; assignment, probing, the spherical Lloyd iterations, the regrouping of a store after an add, the
    probed search loop and their half of save and load."""

    _inverted_table = True       # whether the scan walks the probe table inverted (by list): what ops.ivf_plan makes

    def _init_lists(self, nlist):
        nlist = int(nlist)
        if nlist < 1 or nlist > 65535:
            raise ValueError('1 <= nlist <= 65535 expected, got %d' % nlist)
        self.nlist = nlist
        self.centroids = self.ccodes = self.cscales = None
        self.ids = torch.empty(0, dtype=torch.int32, device='cuda')
        self.list_off = torch.zeros(nlist + 1, dtype=torch.int32, device='cuda')
        self._lens = np.zeros(nlist, np.int64)           # host copy of the list lengths: sizes search's chunks

    def _trained(self):
        return self.centroids is not None and super()._trained()

    def _set_centroids(self, centroids):
        self.centroids = centroids
        self.ccodes, self.cscales = ops.quantize_rows(centroids)

    def _assign(self, codes, scales, scratch_bytes=256 << 20):
        """the list of every coded row [n] int32: the best centroid by quantised score under ops.topk's order"""
        n = codes.shape[0]
        out = torch.empty(n, dtype=torch.int32, device='cuda')
        rows = int(max(1, min(1 << 22, scratch_bytes // (4 * self.nlist))))     # (similarity_i8 takes 65535 * 96 rows a call)
        for r0 in range(0, n, rows):
            scores = ops.similarity_i8(codes[r0:r0 + rows], scales[r0:r0 + rows], self.ccodes, self.cscales, self.D)
            out[r0:r0 + rows] = ops.topk(scores, 1)[0][:, 0]
        return out

    def _lloyd_centroids(self, x, iters, seed):
        """IVFInt8Index.train's iterations on the sample x [n, D] (fp32 CUDA, n >= nlist); sets the centroids"""
        first = np.sort(np.random.RandomState(seed).choice(int(x.shape[0]), self.nlist, replace=False))
        centroids = x[torch.from_numpy(first).cuda()].clone()
        codes, scales = ops.quantize_rows(x)
        bounds = torch.arange(self.nlist + 1, device='cuda')
        for _ in range(int(iters)):
            self._set_centroids(centroids)
            seg_off, sums = _segment_sums(x, self._assign(codes, scales), bounds)
            ops.l2norm_rows_(sums)
            empty = (seg_off[1:] == seg_off[:-1])[:, None]
            centroids = torch.where(empty, centroids, sums)
        self._set_centroids(centroids)

    def train(self, x, iters=10, seed=0, max_rows=None):
        """The train of the inverted files (IVFPQIndex.train goes on from it).  Spherical Lloyd iterations on the rows of x
        [n, D] (any kind add takes), or on a sorted np.random.RandomState(seed).choice sample of max_rows of them (default
        256 * nlist) when x has more.  The initial
        centroids are the rows np.sort(RandomState(seed).choice(n, nlist, replace=False)) of the sample; an iteration
        assigns every row to its list, sums each list's members in fp32 (ops.segment_sums) and L2-normalises the sums;
        an empty list keeps its centroid.  Bitwise reproducible.  Rows already added are not re-assigned: train first."""
        self._check_train(x)
        max_rows = 256 * self.nlist if max_rows is None else int(max_rows)
        self._lloyd_centroids(_training_rows(x, seed, max_rows, self.nlist, 'nlist = %d' % self.nlist), iters, seed)
        return self

    def _add_lists(self, descs, names, encode):
        """The add of an inverted file: every chunk x of ADD_CHUNK_BYTES is quantised to int8 and assigned to its lists,
        encode(x, lists, codes, scales) -> its rows for the stores self.<names>, and the stores are regrouped (_regroup)."""
        self._check_rows(descs)
        self._need_trained('add')
        if int(descs.shape[0]) == 0:
            return self
        lists, stores = [], [[getattr(self, name)] for name in names]
        for x in _row_chunks(descs, self.D):
            c, s = ops.quantize_rows(x)
            lists.append(self._assign(c, s))
            for store, part in zip(stores, encode(x, lists[-1], c, s)):
                store.append(part)
        for name, store in zip(names, self._regroup(lists, [torch.cat(store) for store in stores])):
            setattr(self, name, store)
        return self

    def _regroup(self, new_lists, stores):
        """After n rows were appended: new_lists, their lists (int32 tensors, in add order); stores, the per-row tensors
        with the new rows appended [N + n, ...].  A stable integer sort of the list indices, old rows first, so ids ascend
        inside a list; sets ids, list_off and _lens (one read-back) and returns the regrouped stores."""
        N = int(self.ids.numel())
        n = sum(int(l.numel()) for l in new_lists)
        old_lists = torch.searchsorted(self.list_off[1:].long(), torch.arange(N, device='cuda'), right=True)
        lists, order = torch.sort(torch.cat([old_lists] + [l.long() for l in new_lists]), stable=True)
        self.ids = torch.cat([self.ids, torch.arange(N, N + n, dtype=torch.int32, device='cuda')])[order]
        self.list_off = torch.searchsorted(lists, torch.arange(self.nlist + 1, device='cuda')).to(torch.int32)
        self._lens = np.diff(self.list_off.cpu().numpy().astype(np.int64))
        return [s[order] for s in stores]

    def probe(self, qc, qs, nprobe):
        """the lists of every coded query [Q, nprobe] int32, best first"""
        return ops.topk(ops.similarity_i8(qc, qs, self.ccodes, self.cscales, self.D), nprobe)[0]

    def _slots(self, probe):
        """col_off [Q, nprobe] int32: the probed lists of a query side by side, in probe order"""
        lens = (self.list_off[1:] - self.list_off[:-1])[probe.long()]
        return torch.cumsum(lens, dim=1, dtype=torch.int32) - lens

    def _plan_items(self, rows, nprobe):
        """A host bound of the workgroups a scan by list of `rows` queries at nprobe distinct lists each takes.  List l
        (tiles_l = ceil(len_l / 256)), probed by n_l >= 1 queries of the chunk, takes tiles_l * ceil(n_l / 32) <=
        tiles_l * (n_l + 31) / 32 workgroups.  With T(m) = the tiles of the m longest lists added up: the sum of
        tiles_l * n_l is the sum over the queries of the tiles of their lists, at most rows * T(nprobe); the probed lists
        are at most m = min(nlist, rows * nprobe), their tiles at most T(m).  So (rows * T(nprobe) + 31 * T(m)) / 32 bounds
        the grid - never above the plain rows * T(nprobe), and exact for one query."""
        if getattr(self, '_tiles_of', None) is not self._lens:         # (a new _lens array after every add and load)
            tiles = np.sort((self._lens + 255) // 256)[::-1]
            self._tiles_top, self._tiles_of = np.concatenate([[0], np.cumsum(tiles)]), self._lens
        rows, top = int(rows), self._tiles_top
        return (rows * int(top[nprobe]) + 31 * int(top[min(len(top) - 1, rows * nprobe)])) // 32

    def _search_lists(self, qdescs, k, nprobe, rerank, source, same_set, scratch_bytes, query_bytes, plan='host'):
        """The search of an inverted file around self._scan_lists(q, qc, qs, probe, col_off, rows, width, tables) -> the
        (scores, ids) [len(rows), <= width] of the queries of the slice `rows` against the lists they probe (probe and
        col_off: those of the chunk): the queries go in chunks whose score and id rows (8 bytes per column; the nprobe
        longest lists bound the width, by the host's copy of the list lengths) and query_bytes more per query fit
        scratch_bytes.
        plan: where the tables of a chunk come from.  'host': col_off from integer torch operations and, for the two scans
        by list, the inverted table from ops.ivf_probe_tables, which reads its grid and its width back - one
        synchronisation per chunk.  'device': ops.ivf_plan makes them in one launch, the width is the host's bound above
        and the grid the bound of _plan_items: nothing is read back; a chunk the planner or the launch limit does not take
        (more than ops.ivf_plan_max_pairs() pairs, a bound above ops.ivf_scan_max_items()) is a ValueError.  'auto':
        'device' where the chunks are admissible, else 'host'.  The lists returned are the same bits either way."""
        nprobe = int(nprobe)
        if nprobe < 1 or nprobe > self.nlist:
            raise ValueError('1 <= nprobe <= nlist = %d expected, got %d' % (self.nlist, nprobe))
        if plan not in ('auto', 'device', 'host'):
            raise ValueError("plan: 'auto', 'device' or 'host' expected, got %r" % (plan,))

        def scan(q, keep):
            Q = q.shape[0]
            qc, qs = ops.quantize_rows(q)
            probe = self.probe(qc, qs, nprobe)
            width = max(int(np.partition(self._lens, -nprobe)[-nprobe:].sum()), keep)     # the nprobe longest lists
            step = int(max(1, min(Q, scratch_bytes // (8 * width + query_bytes))))
            planned = plan != 'host' and self._inverted_table
            if planned:         # every chunk has at most `step` queries: the first decides for all
                items = self._plan_items(step, nprobe)
                planned = step * nprobe <= ops.ivf_plan_max_pairs() and items <= ops.ivf_scan_max_items()
                if not planned and plan == 'device':
                    raise ValueError("plan='device': a chunk of %d queries at %d lists has %d pairs and a grid bound of %d; "
                                     "at most %d and %d are planned on the device - lower scratch_bytes or nprobe, or "
                                     "plan='auto'" % (step, nprobe, step * nprobe, items, ops.ivf_plan_max_pairs(),
                                                      ops.ivf_scan_max_items()))
            col_off = None if planned else self._slots(probe)
            cand = torch.empty(Q, keep, dtype=torch.int32, device='cuda')
            vals = torch.empty(Q, keep, dtype=torch.float32, device='cuda')
            for r0 in range(0, Q, step):
                r1 = min(Q, r0 + step)
                if planned:
                    slots, tables, _ = ops.ivf_plan(self.list_off, probe[r0:r1], self._plan_items(r1 - r0, nprobe))
                else:
                    slots, tables = col_off[r0:r1], None
                scores, ids = self._scan_lists(q, qc, qs, probe[r0:r1], slots, slice(r0, r1), width, tables)
                if scores.shape[1] < keep:   # every row of the chunk runs short: top-k wants keep columns, the rest are empty
                    wide = torch.full((r1 - r0, keep), -1, dtype=torch.int32, device='cuda')
                    wide[:, :ids.shape[1]] = ids
                    ids, scores = wide, torch.cat([scores, scores.new_zeros(r1 - r0, keep - scores.shape[1])], dim=1)
                own = torch.arange(r0, r1, dtype=torch.int32, device='cuda') if same_set else None
                cand[r0:r1], vals[r0:r1] = ops.topk(scores, keep, ids=ids, exclude=own)
            return cand, vals
        return self._search(qdescs, k, rerank, source, same_set, scratch_bytes, scan)

    def _save_lists(self):
        """the lists' arrays of a .npz: `centroids` [nlist, D] float32, `ids` [N] int32, `list_off` [nlist+1] int32, `nlist`"""
        return dict(centroids=self.centroids.cpu().numpy(), ids=self.ids.cpu().numpy(), list_off=self.list_off.cpu().numpy(),
                    nlist=np.int64(self.nlist))

    def _load_lists(self, path, f):
        """after the code store is loaded: N is its row count"""
        N, centroids, ids, list_off = len(self), f['centroids'], f['ids'], f['list_off']
        if ids.shape != (N,):
            raise ValueError('%s: ids [N] expected for codes of N rows' % path)
        if centroids.shape != (self.nlist, self.D) or list_off.shape != (self.nlist + 1,) or list_off[0] != 0 or (
                list_off[-1] != N or (np.diff(list_off.astype(np.int64)) < 0).any()):
            raise ValueError('%s: centroids [nlist, D] and a list_off [nlist+1] from 0 to N expected' % path)
        self._set_centroids(torch.from_numpy(centroids.astype(np.float32)).cuda())
        self.ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        self.list_off = torch.from_numpy(list_off.astype(np.int32)).cuda()
        self._lens = np.diff(list_off.astype(np.int64))


class _ProductQuantizer:
    """What the two product-quantised indexes share: M sub-spaces of dsub = D / M columns, codebooks [M, 256, dsub] fp32
    (None until train or load), the uint8 code store [N, M rounded up to 4] (padding zero) in place of the int8 one, the
    Lloyd iterations per sub-space and their half of save and load."""

    def _init_pq(self, M):
        M = int(M)
        if M < 1 or M > ops.pq_max_m() or self.D % M:
            raise ValueError('1 <= M <= %d dividing D = %d expected, got %d' % (ops.pq_max_m(), self.D, M))
        self.M, self.dsub = M, self.D // M
        self.codebooks = None
        self.codes = torch.empty(0, _round_up(M, 4), dtype=torch.uint8, device='cuda')
        self.scales = None

    def _trained(self):
        return self.codebooks is not None and super()._trained()

    def _lloyd_codebooks(self, x, iters, seed):
        """PQIndex.train's iterations on the sample x [n, D] (fp32 CUDA, n >= 256); sets the codebooks"""
        M, dsub = self.M, self.dsub
        first = np.sort(np.random.RandomState(seed).choice(int(x.shape[0]), 256, replace=False))
        codebooks = x[torch.from_numpy(first).cuda()].view(256, M, dsub).permute(1, 0, 2).contiguous()
        bounds = torch.arange(257, device='cuda')
        for _ in range(int(iters)):
            codes = ops.pq_encode(x, codebooks)
            for m in range(M):
                seg_off, sums = _segment_sums(x[:, m * dsub:(m + 1) * dsub], codes[:, m], bounds)
                count = (seg_off[1:] - seg_off[:-1])[:, None]
                codebooks[m] = torch.where(count > 0, sums / count.to(torch.float32), codebooks[m])
        self.codebooks = codebooks

    def _save_pq(self):
        """the quantiser's arrays of a .npz: `codebooks` [M, 256, D / M] float32, `codes` [N, M] uint8 (without the
        padding), `M`"""
        return dict(codebooks=self.codebooks.cpu().numpy(), codes=self.codes[:, :self.M].cpu().numpy(), M=np.int64(self.M))

    def _load_pq(self, path, f):
        codebooks = f['codebooks']
        if codebooks.shape != (self.M, 256, self.dsub) or codebooks.dtype.kind != 'f':
            raise ValueError('%s: codebooks [M, 256, D / M] float32 expected' % path)
        self.codes = _padded_codes(path, f['codes'], self.M, np.uint8, 4)
        self.codebooks = torch.from_numpy(np.ascontiguousarray(codebooks, dtype=np.float32)).cuda()


class _InvertedFile(_InvertedLists, _CodedIndex):
    """The constructor, nbytes, save and load of the three inverted files over a code store (`_store`); a class adds its add,
    its _scan_lists and its search."""

    def __init__(self, D, nlist):
        _CodedIndex.__init__(self, D)
        self._init_lists(nlist)

    def nbytes(self):
        """the bytes the database rows take on the device: the store's tensors and ids (centroids not counted)"""
        return sum(int(t.numel()) * t.element_size() for t in self._stored() + [self.ids])

    def save(self, path):
        """One .npz: the arrays of the flat index over the same store (`D` with them) and the lists' (`centroids` [nlist, D]
        float32, `ids` [N] int32, `list_off` [nlist+1] int32, `nlist`).  The flat class's load reads the file as it lies: the
        rows list-major, without their ids."""
        self._need_trained('save')
        np.savez(path, D=np.int64(self.D), **self._store.save(self), **self._save_lists())

    @classmethod
    def load(cls, path):
        f = _read_npz(path)
        index = cls(int(f['D']), int(f['nlist']))
        index._load_store(path, f)
        index._load_lists(path, f)
        return index


class IVFInt8Index(_InvertedFile):
    """The inverted-file int8 index (include/dir_engine.h gives the definitions).  All CUDA: centroids [nlist, D] fp32 with
    their codes `ccodes` and scales `cscales`; the database LIST-MAJOR - codes [N, ldc] int8, scales [N] fp32, ids [N] int32
    (a row's number in add order: what Int8Index reports) - and list_off [nlist+1] int32, a CSR from 0 to N; inside a list
    the rows are in ascending id.  save: one .npz of `centroids` [nlist, D] float32, `codes` [N, D] int8 (without the
    padding), `scales` [N] float32, `ids` [N] int32, `list_off` [nlist+1] int32, `D`, `nlist`."""

    def add(self, descs):
        """Append the rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap), quantised in chunks of
        ADD_CHUNK_BYTES as Int8Index.add does; their ids continue the count.  The store is regrouped by a stable integer
        sort of the list indices (old rows first, so ids ascend inside a list): what the index holds does not depend on
        how the rows were cut into calls.  The regrouping copies the codes once (twice the index's bytes for a moment)
        and reads the list lengths back to the host."""
        return self._add_lists(descs, ('codes', 'scales'), lambda x, lists, c, s: (c, s))

    def _scan_lists(self, q, qc, qs, probe, col_off, rows, width, tables):
        return ops.ivf_scan(qc[rows], qs[rows], self.codes, self.scales, self.ids, self.list_off, probe, col_off, self.D,
                            width=None if tables is None else width, tables=tables)

    def search(self, qdescs, k, nprobe=1, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, plan=DEFAULT_PLAN):
        """Int8Index.search's contract over the rows of the nprobe best lists of every query (1 <= nprobe <= nlist): a
        query whose lists hold fewer than k rows ends in (-1, NaN).  The queries go in chunks whose score and id rows
        (8 bytes per column; the nprobe longest lists bound the width) fit scratch_bytes.  plan (_search_lists gives the
        rules): with 'host' every chunk synchronises with the host once, inside ops.ivf_scan, to learn its grid and its
        width; with 'device' - and with 'auto' wherever the chunks are admissible - ops.ivf_plan makes the probe tables in
        one launch, grid and width are host bounds, and with queries (and a rerank source) on the device the search
        never waits for the host.  The lists are the same bits."""
        return self._search_lists(qdescs, k, nprobe, rerank, source, same_set, scratch_bytes, 0, plan)


class IVFFp4Index(_InvertedFile):
    """The inverted file over fp4 codes (include/dir_engine.h gives the definitions; numpy restatement: tests/ivffp4_ref.py).
    All CUDA: IVFInt8Index's coarse quantiser (centroids [nlist, D] fp32, `ccodes`, `cscales`: assignment and probing by the
    int8 score, so a row lands in the list IVFInt8Index puts it in) and the database LIST-MAJOR as Fp4Index stores a row -
    codes [N, ldc] uint8, exps [N, lde] uint8, scales [N] fp32, (ldc, lde) = ops.fp4_widths(D) - with ids [N] int32 and
    list_off [nlist+1] int32; inside a list the rows are in ascending id.  save: one .npz of Fp4Index's arrays and the
    lists'."""
    _store = _Fp4Store

    def add(self, descs):
        """IVFInt8Index.add's contract: a chunk of ADD_CHUNK_BYTES is quantised to int8 for its assignment and to fp4 for
        the store, and the three stores are regrouped by that class's stable integer sort, so what the index holds does
        not depend on how the rows were cut into calls."""
        return self._add_lists(descs, ('codes', 'exps', 'scales'), lambda x, lists, c, s: ops.quantize_rows_fp4(x))

    def _scan_lists(self, q, qc, qs, probe, col_off, rows, width, tables):
        fc, fe, fs = ops.quantize_rows_fp4(q[rows])
        return ops.ivf_scan_fp4(fc, fe, fs, self.codes, self.exps, self.scales, self.ids, self.list_off, probe, col_off,
                                self.D, width=None if tables is None else width, tables=tables)

    def search(self, qdescs, k, nprobe=1, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, plan=DEFAULT_PLAN):
        """IVFInt8Index.search's contract with the fp4 scores in place of the int8 ones: the lists of a query are probed by
        its int8 codes, their rows scored by its fp4 codes; a query whose lists hold fewer than k rows ends in (-1, NaN).
        The queries go in chunks whose score and id rows (8 bytes per column) and fp4 codes fit scratch_bytes.  plan as
        in IVFInt8Index.search: 'host' synchronises once per chunk, inside ops.ivf_scan_fp4; 'device' (and 'auto' where
        admissible) plans the chunk with ops.ivf_plan and does not."""
        ldc, lde = ops.fp4_widths(self.D)
        return self._search_lists(qdescs, k, nprobe, rerank, source, same_set, scratch_bytes, ldc + lde + 4, plan)


class IVFBinaryIndex(_InvertedFile):
    """The inverted file over sign-bit rows (include/dir_engine.h gives the definitions; numpy restatement:
    tests/ivfbin_ref.py).  All CUDA: IVFInt8Index's coarse quantiser (centroids [nlist, D] fp32, `ccodes`, `cscales`:
    assignment and probing by the int8 score, so a row lands in the list IVFInt8Index puts it in) and the database LIST-MAJOR
    as BinaryIndex stores a row - codes [N, ops.bin_width(D)] uint8, scales [N] fp32 - with ids [N] int32 and list_off
    [nlist+1] int32; inside a list the rows are in ascending id.  Its raw lists are coarse: pair it with rerank.  save: one
    .npz of BinaryIndex's arrays and the lists'; BinaryIndex.load reads the file as it lies, the rows list-major, without
    their ids."""
    _store = _BinStore

    def add(self, descs):
        """IVFInt8Index.add's contract: a chunk of ADD_CHUNK_BYTES is quantised to int8 for its assignment and to sign bits
        for the store, and the two stores are regrouped by that class's stable integer sort, so what the index holds does
        not depend on how the rows were cut into calls."""
        return self._add_lists(descs, ('codes', 'scales'), lambda x, lists, c, s: ops.quantize_rows_bin(x))

    def _scan_lists(self, q, qc, qs, probe, col_off, rows, width, tables):
        # the int8 codes that probed the lists score their rows too: only their sums are new
        return ops.ivf_scan_bin(qc[rows], qs[rows], self.codes, self.scales, self.ids, self.list_off, probe, col_off, self.D,
                                width=None if tables is None else width, tables=tables, qsums=ops.code_sums(qc[rows], self.D))

    def search(self, qdescs, k, nprobe=1, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, plan=DEFAULT_PLAN):
        """IVFInt8Index.search's contract with the sign-bit scores in place of the int8 ones: the lists of a query are
        probed and their rows scored by the same int8 codes; a query whose lists hold fewer than k rows ends in (-1, NaN).
        The queries go in chunks whose score and id rows (8 bytes per column) and code sums fit scratch_bytes.  plan as in
        IVFInt8Index.search: 'host' synchronises once per chunk, inside ops.ivf_scan_bin; 'device' (and 'auto' where
        admissible) plans the chunk with ops.ivf_plan and does not."""
        return self._search_lists(qdescs, k, nprobe, rerank, source, same_set, scratch_bytes, 4, plan)


class PQIndex(_ProductQuantizer, _CodedIndex):
    """The product-quantised index (include/dir_engine.h gives the definitions).  All CUDA: codebooks [M, 256, D / M] fp32
    (None until train or load) and codes [N, ldc] uint8, ldc = M rounded up to a multiple of 4, the padding zero."""

    def __init__(self, D, M):
        _CodedIndex.__init__(self, D)
        self._init_pq(M)

    def nbytes(self):
        """the bytes the database rows take on the device (the codebooks, 1024 * D bytes, not counted)"""
        return len(self) * int(self.codes.shape[1])

    def train(self, x, iters=10, seed=0, max_rows=None):
        """Lloyd iterations per sub-space on the rows of x [n, D] (any kind add takes), or on a sorted
        np.random.RandomState(seed).choice sample of max_rows of them (default 256 * 256) when x has more.  The initial
        centroids are the rows np.sort(RandomState(seed).choice(n, 256, replace=False)) of the sample, sub-space m taking
        its columns of them; an iteration encodes the sample (ops.pq_encode is the assignment), sums each centroid's
        members in fp32 (ops.segment_sums on the sub-space's columns) and divides by their number; a centroid without
        members keeps its value.  Bitwise reproducible.  Rows already added are not re-encoded: train first."""
        self._check_train(x)
        max_rows = 256 * 256 if max_rows is None else int(max_rows)
        self._lloyd_codebooks(_training_rows(x, seed, max_rows, 256, '256'), iters, seed)
        return self

    def add(self, descs):
        """Append the rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap), encoded in chunks of
        ADD_CHUNK_BYTES as Int8Index.add quantises them."""
        self._check_rows(descs)
        self._need_trained('add')
        if int(descs.shape[0]):
            self.codes, = _appended([self.codes], descs, self.D, lambda x: [ops.pq_encode(x, self.codebooks)])
        return self

    def search(self, qdescs, k, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, db_rows=None):
        """Int8Index.search's contract with the table scores in place of the quantised ones: (idx [Q,k] int32, vals [Q,k]
        float32), both CUDA, in ops.topk's order, same_set leaving a query out of its own list, (-1, NaN) where a row runs
        short; rerank = R re-scores the R best against `source` (CUDA tensor, host array or memmap) in fp32.  A chunk of
        queries holds its tables, 1024 * M bytes each, beside its score rows."""
        def scan(q, keep):
            def scorer(r0, r1):
                lut = ops.pq_lut(q[r0:r1], self.codebooks)
                return lambda b0, b1: ops.pq_scan(lut, self.codes[b0:b1])
            return self._scan_blocks(q.shape[0], keep, same_set, scratch_bytes, db_rows, scorer, row_bytes=1024 * self.M)
        return self._search(qdescs, k, rerank, source, same_set, scratch_bytes, scan)

    def save(self, path):
        """One .npz: `codebooks` [M, 256, D / M] float32, `codes` [N, M] uint8 (without the padding), `D`, `M`."""
        self._need_trained('save')
        np.savez(path, D=np.int64(self.D), **self._save_pq())

    @classmethod
    def load(cls, path):
        f = _read_npz(path)
        index = cls(int(f['D']), int(f['M']))
        index._load_pq(path, f)
        return index


class IVFPQIndex(_InvertedLists, _ProductQuantizer, _CodedIndex):
    """The IVF-PQ index (include/dir_engine.h gives the definitions).  All CUDA: the coarse quantiser of IVFInt8Index
    (centroids [nlist, D] fp32, `ccodes`, `cscales`), codebooks [M, 256, D / M] fp32 trained on residuals, and the database
    LIST-MAJOR - codes [N, ldc] uint8 (ldc = M rounded up to a multiple of 4, the padding zero): the codes of the row's
    residual to the fp32 centroid of its list; ids [N] int32; list_off [nlist+1] int32, a CSR from 0 to N; inside a list
    the rows are in ascending id."""

    def __init__(self, D, nlist, M):
        _CodedIndex.__init__(self, D)
        self._init_lists(nlist)
        self._init_pq(M)

    def nbytes(self):
        """the bytes the database rows take on the device: codes and ids (centroids and codebooks not counted)"""
        return len(self) * (int(self.codes.shape[1]) + 4)

    def _residuals(self, x, lists):
        """x [n, D] fp32 CUDA minus the fp32 centroid of every row's list: one subtraction per element"""
        return x - self.centroids[lists.long()]

    def train(self, x, iters=10, seed=0, max_rows=None):
        """Two steps on the rows of x [n, D] (any kind add takes), or on IVFInt8Index.train's sample of max_rows of them
        (default 256 * nlist) when x has more; at least max(nlist, 256) rows.  1. the coarse centroids exactly as
        IVFInt8Index.train finds them.  2. the codebooks exactly as PQIndex.train finds them (same seed, same iterations),
        but on the residuals of that sample to the final centroids of the lists its rows are assigned to.  Bitwise
        reproducible.  Rows already added are neither re-assigned nor re-encoded: train first."""
        self._check_train(x)
        max_rows = 256 * self.nlist if max_rows is None else int(max_rows)
        least = max(self.nlist, 256)
        x = _training_rows(x, seed, max_rows, least, 'max(nlist, 256) = %d' % least)
        self._lloyd_centroids(x, iters, seed)
        self._lloyd_codebooks(self._residuals(x, self._assign(*ops.quantize_rows(x))), iters, seed)
        return self

    def add(self, descs):
        """Append the rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap) in chunks of ADD_CHUNK_BYTES:
        a chunk is quantised and assigned as IVFInt8Index.add does, its residuals are encoded (ops.pq_encode), and the
        store is regrouped by that class's stable integer sort, so what the index holds does not depend on how the rows
        were cut into calls."""
        return self._add_lists(descs, ('codes',),
                               lambda x, lists, c, s: [ops.pq_encode(self._residuals(x, lists), self.codebooks)])

    _inverted_table = False      # the scan is cut query-major: it reads probe and col_off as they are

    def _scan_lists(self, q, qc, qs, probe, col_off, rows, width, tables):
        lut = ops.pq_lut(q[rows], self.codebooks)
        base = ops.ivfpq_base(q[rows], self.centroids, probe, self.M)
        return ops.ivfpq_scan(lut, base, self.codes, self.ids, self.list_off, probe, col_off, width=width)

    def search(self, qdescs, k, nprobe=1, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, plan=DEFAULT_PLAN):
        """IVFInt8Index.search's contract over the rows of the nprobe best lists of every query (1 <= nprobe <= nlist), with
        the score  <q, centroid of the list> + the row's table entries  in place of the quantised one; a query whose lists
        hold fewer than k rows ends in (-1, NaN).  The queries go in chunks whose score and id rows (8 bytes per column;
        the nprobe longest lists give the width) and tables (1024 * M bytes per query) fit scratch_bytes.  The width comes
        from the host's copy of the list lengths: a search does not synchronise with the host.  plan is taken (and
        checked) for one interface over the three inverted files and changes nothing here: this scan walks no inverted
        table, and its col_off stays the four integer torch launches of every plan."""
        return self._search_lists(qdescs, k, nprobe, rerank, source, same_set, scratch_bytes, 1024 * self.M, plan)

    def save(self, path):
        """One .npz: `centroids` [nlist, D] float32, `codebooks` [M, 256, D / M] float32, `codes` [N, M] uint8 (without the
        padding), `ids` [N] int32, `list_off` [nlist+1] int32, `D`, `nlist`, `M`."""
        self._need_trained('save')
        np.savez(path, D=np.int64(self.D), **self._save_pq(), **self._save_lists())

    @classmethod
    def load(cls, path):
        f = _read_npz(path)
        index = cls(int(f['D']), int(f['nlist']), int(f['M']))
        index._load_pq(path, f)
        index._load_lists(path, f)
        return index

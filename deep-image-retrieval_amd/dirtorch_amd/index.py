"""The int8 descriptor index: a database kept as per-row int8 codes with one fp32 scale per row (a quarter of the fp32
bytes), scanned on the int8 matrix cores and, on request, re-ranked with the full-precision rows.

    index = Int8Index(D)
    index.add(bdescs)                                        # CUDA / CPU tensor, ndarray or memmap: quantised in row chunks
    idx, vals = index.search(qdescs, 10)                     # lists by quantised score
    idx, vals = index.search(qdescs, 10, rerank=40, source=bdescs)   # shortlist of 40, re-scored in fp32, then the 10 best

include/dir_engine.h defines the quantisation and the quantised score; an int8 dot product accumulated in int32 is exact,
so a quantised score is one defined fp32 number and the lists of a scan do not depend on scratch_bytes, db_rows or on how
many add() calls built the database.
"""
import numpy as np
import torch

from . import ops

ADD_CHUNK_BYTES = 256 << 20     # fp32 bytes of a database that are on the device at a time while it is quantised


def _pad64(D):
    return (D + 63) // 64 * 64


def _is_host(x):
    return isinstance(x, np.ndarray) or (torch.is_tensor(x) and not x.is_cuda)


def _upload(x):
    """rows of an ndarray / memmap / tensor -> contiguous fp32 CUDA tensor"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return x.to(device='cuda', dtype=torch.float32).contiguous()


class Int8Index:
    """codes [N, ldc] int8 (ldc = D rounded up to 64, padding zero) and scales [N] fp32, both CUDA."""

    def __init__(self, D):
        D = int(D)
        if D < 1 or D > ops.index_i8_max_dim():
            raise ValueError('1 <= D <= %d expected, got %d' % (ops.index_i8_max_dim(), D))
        self.D = D
        self.codes = torch.empty(0, _pad64(D), dtype=torch.int8, device='cuda')
        self.scales = torch.empty(0, dtype=torch.float32, device='cuda')

    def __len__(self):
        return int(self.codes.shape[0])

    def add(self, descs):
        """Append the rows of descs [n, D] (fp32 CUDA tensor, CPU tensor, ndarray or memmap).  They are quantised in
        chunks of ADD_CHUNK_BYTES, so a database that lives in a host file is never resident on the device as fp32."""
        if descs.ndim != 2 or descs.shape[1] != self.D:
            raise ValueError('descriptors [n, %d] expected' % self.D)
        n, N = int(descs.shape[0]), len(self)
        if n == 0:
            return self
        codes = torch.empty(N + n, self.codes.shape[1], dtype=torch.int8, device='cuda')
        scales = torch.empty(N + n, dtype=torch.float32, device='cuda')
        codes[:N], scales[:N] = self.codes, self.scales
        rows = max(1, ADD_CHUNK_BYTES // (4 * self.D))
        for r0 in range(0, n, rows):
            r1 = min(n, r0 + rows)
            codes[N + r0:N + r1], scales[N + r0:N + r1] = ops.quantize_rows(_upload(descs[r0:r1]))
        self.codes, self.scales = codes, scales
        return self

    def _scan(self, qc, qs, keep, same_set, scratch_bytes, db_rows):
        """ranking.retrieve_device's loop on the coded sets: the `keep` best rows of every query by quantised score."""
        Q, N = qc.shape[0], len(self)
        block = N if db_rows is None else int(max(keep, min(N, db_rows)))
        idx = torch.empty(Q, keep, dtype=torch.int32, device='cuda')
        vals = torch.empty(Q, keep, dtype=torch.float32, device='cuda')
        rows = int(max(1, min(Q, scratch_bytes // max(4 * block, 1))))
        for r0 in range(0, Q, rows):
            r1 = min(Q, r0 + rows)
            own = torch.arange(r0, r1, dtype=torch.int32, device='cuda') if same_set else None
            run_i = run_v = None
            for b0 in range(0, N, block):
                b1 = min(N, b0 + block)
                scores = ops.similarity_i8(qc[r0:r1], qs[r0:r1], self.codes[b0:b1], self.scales[b0:b1], self.D)
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

    def search(self, qdescs, k, rerank=0, source=None, same_set=False, scratch_bytes=256 << 20, db_rows=None):
        """(idx [Q,k] int32, vals [Q,k] float32), both CUDA, under ranking.retrieve_device's contract (its order, same_set
        leaving a query out of its own list, (-1, NaN) where a row runs short).  rerank = 0: ranked by the quantised
        scores, which vals carries.  rerank = R, k <= R <= min(N, ops.topk_max_k()): the scan keeps the R best per query,
        they are re-scored against `source` - the fp32 database: a CUDA tensor is gathered on the device, a host array
        or memmap has the candidates' rows gathered on the host in chunks of scratch_bytes - and vals carries the fp32
        scores of the k best of them."""
        from .utils.common import _dev
        q = _dev(qdescs)
        Q, N = q.shape[0], len(self)
        k, R = int(k), int(rerank)
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
        qc, qs = ops.quantize_rows(q)
        cand, vals = self._scan(qc, qs, R or k, same_set, scratch_bytes, db_rows)
        if not R:
            return cand, vals
        return ops.topk(self._rescore(q, cand, source, scratch_bytes), k, ids=cand)

    def save(self, path):
        """One .npz: `codes` [N, D] int8 (without the padding), `scales` [N] float32, `D`."""
        np.savez(path, codes=self.codes[:, :self.D].cpu().numpy(), scales=self.scales.cpu().numpy(),
                 D=np.int64(self.D))

    @classmethod
    def load(cls, path):
        with np.load(path) as f:
            index = cls(int(f['D']))
            codes, scales = f['codes'], f['scales']
        if codes.dtype != np.int8 or codes.ndim != 2 or codes.shape[1] != index.D or scales.shape != (len(codes),):
            raise ValueError('%s: codes [N, D] int8 and scales [N] expected' % path)
        index.codes = torch.zeros(len(codes), _pad64(index.D), dtype=torch.int8, device='cuda')
        index.codes[:, :index.D] = torch.from_numpy(codes).cuda()
        index.scales = torch.from_numpy(scales.astype(np.float32)).cuda()
        return index

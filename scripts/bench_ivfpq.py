#!/usr/bin/env python
"""The IVF-PQ index on one MI355X beside the two indexes it composes - PQIndex (same M, every row scanned) and IVFInt8Index
(same lists, D bytes a row) - on bench_index.py's seeded unit-norm descriptors.
    python scripts/bench_ivfpq.py [--shapes 1006322 20000] [--d 2048] [--m 64 128] [--nlist 1024] [--nprobe 1 8 32]
                                  [--q 1 70] [--k 10 100] [--clusters 16384 6] [--out profiles/ivfpq.txt]
For every database size N (a size of at most 2^17 rows is also searched with itself as the query set: same_set), every
cluster count and every M:
  bytes held     the database rows of the three indexes
  train, add     IVFPQIndex.train (the inverted file's sample, `--iters` iterations for the lists and for the codebooks) and
                 add, once each, beside the other two (synchronised wall clock)
  scan           ops.ivfpq_scan alone on prepared tables, coarse terms and slots, beside ops.pq_scan of the same queries
                 over every row (same M) and ops.ivf_scan over the same lists (probe tables prepared): device events, the
                 three alternating inside every repeat; ops.pq_lut and ops.ivfpq_base, which an IVF-PQ search pays per
                 query, on their own line
  search         descriptors -> lists at every k, rerank = 0 and rerank = 4k (CUDA source): IVFPQIndex.search and
                 IVFInt8Index.search at every nprobe and PQIndex.search, all alternating inside every repeat (synchronised
                 wall clock)
  recall@k       of IVFPQIndex's lists against ranking.retrieve_device's (fp32 rows) and against PQIndex's lists of the same
                 rerank; IVFInt8Index's and PQIndex's own recall against the fp32 lists beside them
Every timing is the median (min .. max) of `--repeats` after a warm-up.  Nothing here is a gate: the figures are reported as
measured, the cases IVF-PQ loses included.  The queries of a Q x N shape with Q != N are further rows of the database's own
draw (bench_ivf.py explains why), so they have relatives in it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import numpy as np
import torch
from bench_index import alternating, descriptors, event_ms, recall, wall_ms
from dirtorch_amd import ops, ranking
from dirtorch_amd.index import IVFInt8Index, IVFPQIndex, PQIndex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=int, nargs='+', default=[1006322, 20000])
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--m', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--nlist', type=int, default=1024)
    ap.add_argument('--nprobe', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--q', type=int, nargs='+', default=[1, 70])
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--clusters', type=int, nargs='+', default=[16384, 6])
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    D, nlist = args.d, args.nlist
    say('# IVF-PQ index beside PQIndex and IVFInt8Index: D = %d, nlist = %d; medians (min .. max) of %d timings after a warm-up'
        % (D, nlist, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for N in args.shapes:
        for clusters in args.clusters:
            centres = torch.randn(clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
            square = N <= 1 << 17
            # (at most 2^17 rows come from synth_descriptors, whose draw depends on the row count: one draw of N + Q rows)
            extra = 0 if square else max(args.q)
            b = descriptors(N + extra, D, 6, centres, clusters=clusters)
            b, qall = b[:N], (b[:N] if square else b[N:].clone())
            qsets = [(Q, qall[:Q], False) for Q in args.q if Q <= len(qall)] + ([(N, b, True)] if square else [])
            ivf = IVFInt8Index(D, nlist)
            t_ivf = wall_ms(lambda: ivf.train(b, iters=args.iters)), wall_ms(lambda: ivf.add(b))
            lens = ivf._lens
            say('## N = %d, %d cluster centres: list sizes %d .. %d, median %d' % (N, clusters, lens.min(), lens.max(), int(np.median(lens))))
            say('IVFInt8Index: train %.1f ms, add %.1f ms, %d bytes held' % (t_ivf[0], t_ivf[1], N * (ivf.codes.shape[1] + 8)))
            exact = {(Q, k): ranking.retrieve_device(q, b, k, same_set=same)[0] for Q, q, same in qsets for k in args.k}
            for M in args.m:
                pq, index = PQIndex(D, M), IVFPQIndex(D, nlist, M)
                t_pq = wall_ms(lambda: pq.train(b, iters=args.iters)), wall_ms(lambda: pq.add(b))
                t_ix = wall_ms(lambda: index.train(b, iters=args.iters)), wall_ms(lambda: index.add(b))
                assert torch.equal(index.list_off, ivf.list_off) and torch.equal(index.ids, ivf.ids)
                say('### M = %d' % M)
                say('IVFPQIndex: train %.1f ms, add %.1f ms, %d bytes held (%d a row + a 4-byte id) | PQIndex: train %.1f ms, add '
                    '%.1f ms, %d bytes held' % (t_ix[0], t_ix[1], index.nbytes(), index.codes.shape[1], t_pq[0], t_pq[1], pq.nbytes()))
                res = {'n': N, 'd': D, 'm': M, 'nlist': nlist, 'clusters': clusters, 'train_ms': t_ix[0], 'add_ms': t_ix[1],
                       'bytes': index.nbytes(), 'points': []}
                for Q, q, same in qsets:
                    qc, qs = ops.quantize_rows(q)
                    chunk = int(max(1, min(Q, (1 << 31) // (4 * N + 1024 * M))))     # queries whose flat scores and tables fit 2 GiB
                    lut = ops.pq_lut(q[:chunk], index.codebooks)
                    flat_out = torch.empty(chunk, N, dtype=torch.float32, device='cuda')
                    tl, = alternating([lambda: ops.pq_lut(q[:chunk], index.codebooks)], args.repeats, lambda fn: event_ms(fn, args.inner))
                    tf, = alternating([lambda: ops.pq_scan(lut, pq.codes, out=flat_out)], args.repeats, lambda fn: event_ms(fn, args.inner))
                    say('Q = %d%s (the scans below take %d queries): pq_lut %.4f ms (%.4f .. %.4f); pq_scan over every row %.4f ms '
                        '(%.4f .. %.4f)' % (Q, ' (same_set)' if same else '', chunk, tl[0], tl[1], tl[2], tf[0], tf[1], tf[2]))
                    del flat_out
                    for nprobe in [p for p in args.nprobe if p <= nlist]:
                        probe = index.probe(qc[:chunk], qs[:chunk], nprobe)
                        col_off = index._slots(probe)
                        tables = ops.ivf_probe_tables(ivf.list_off, probe, col_off)
                        width = max(tables[5], 1)
                        base = ops.ivfpq_base(q[:chunk], index.centroids, probe, M)
                        out = (torch.empty(chunk, width, dtype=torch.float32, device='cuda'),
                               torch.empty(chunk, width, dtype=torch.int32, device='cuda'))
                        cand = int((index.list_off[1:] - index.list_off[:-1])[probe.long()].sum())
                        tb, = alternating([lambda: ops.ivfpq_base(q[:chunk], index.centroids, probe, M)], args.repeats,
                                          lambda fn: event_ms(fn, args.inner))
                        ts, ti = alternating([lambda: ops.ivfpq_scan(lut, base, index.codes, index.ids, index.list_off, probe, col_off,
                                                                     width=width, out=out),
                                              lambda: ops.ivf_scan(qc[:chunk], qs[:chunk], ivf.codes, ivf.scales, ivf.ids, ivf.list_off,
                                                                   probe, col_off, D, width=width, out=out, tables=tables)],
                                             args.repeats, lambda fn: event_ms(fn, args.inner))
                        say('  nprobe = %2d  ivfpq_scan %8.4f ms (%.4f .. %.4f), %d candidates, width %d, %d workgroups | ivf_scan %8.4f '
                            'ms (%.4f .. %.4f) | pq_scan %8.4f ms | ivfpq_base %.4f ms | ivfpq_scan = %.3f of ivf_scan, %.3f of pq_scan'
                            % (nprobe, ts[0], ts[1], ts[2], cand, width, chunk * ((width + 1023) // 1024), ti[0], ti[1], ti[2], tf[0],
                               tb[0], ts[0] / ti[0], ts[0] / tf[0]))
                        res['points'].append({'q': Q, 'scan_q': chunk, 'nprobe': nprobe, 'ivfpq_scan_ms': ts[0], 'ivf_scan_ms': ti[0],
                                              'pq_scan_ms': tf[0], 'pq_lut_ms': tl[0], 'ivfpq_base_ms': tb[0], 'candidates': cand})
                        del out, base, tables
                    del lut
                    nprobes = [p for p in args.nprobe if p <= nlist]
                    for k in args.k:
                        for R in (0, 4 * k):
                            kw = dict(rerank=R, source=b if R else None, same_set=same)
                            fns = [lambda p=p: index.search(q, k, nprobe=p, **kw) for p in nprobes]
                            fns += [lambda p=p: ivf.search(q, k, nprobe=p, **kw) for p in nprobes]
                            fns += [lambda: pq.search(q, k, **kw)]
                            t = alternating(fns, args.repeats, wall_ms)
                            tp = t[-1]
                            pq_exact = recall(tp[3][0], exact[(Q, k)])
                            say('  k = %3d rerank = %3d  PQIndex.search %9.3f ms (%.3f .. %.3f), recall@%d vs fp32 %.4f'
                                % (k, R, tp[0], tp[1], tp[2], k, pq_exact))
                            for j, p in enumerate(nprobes):
                                tx, tv = t[j], t[len(nprobes) + j]
                                r_exact, r_pq = recall(tx[3][0], exact[(Q, k)]), recall(tx[3][0], tp[3][0])
                                v_exact = recall(tv[3][0], exact[(Q, k)])
                                say('      nprobe = %2d  IVFPQIndex.search %9.3f ms (%.3f .. %.3f) | IVFInt8Index.search %9.3f ms (%.3f .. '
                                    '%.3f) | %.3f of it, %.3f of PQIndex; recall@%d: IVF-PQ vs fp32 %.4f, vs PQIndex lists %.4f, '
                                    'IVFInt8Index vs fp32 %.4f' % (p, tx[0], tx[1], tx[2], tv[0], tv[1], tv[2], tx[0] / tv[0],
                                                                   tx[0] / tp[0], k, r_exact, r_pq, v_exact))
                                res['points'].append({'q': Q, 'k': k, 'rerank': R, 'nprobe': p, 'ivfpq_search_ms': tx[0],
                                                      'ivf_search_ms': tv[0], 'pq_search_ms': tp[0], 'recall_fp32': r_exact,
                                                      'recall_pq_lists': r_pq, 'ivf_recall_fp32': v_exact, 'pq_recall_fp32': pq_exact})
                    del qc, qs
                results.append(res)
                del pq, index
            del ivf, b, qall, qsets, exact
            torch.cuda.empty_cache()
    print(json.dumps(results))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

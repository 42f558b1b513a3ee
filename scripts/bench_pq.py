#!/usr/bin/env python
"""The product-quantised index on one MI355X beside the int8 index it shrinks, on seeded unit-norm descriptors.
    python scripts/bench_pq.py [--shapes 70x1006322 20000x20000] [--d 2048] [--m 64 128] [--k 10 100] [--out profiles/pq.txt]
For every shape (Q x N) and every M:
  bytes held        the database rows of PQIndex and of Int8Index (codes + scales), and their ratio - M / D of the int8 codes
  train, add        PQIndex.train (a sample of at most 65536 rows, 10 iterations) and PQIndex.add of the N rows, once each
                    (synchronised wall clock; the first call of a process carries the module load)
  scan              ops.pq_scan alone beside ops.similarity_i8 alone, both writing Q x N fp32 scores, alternating inside every
                    repeat (device events); ops.pq_lut of the Q queries on its own line; and the same pq_scan over codes
                    that are all equal - the same instructions with every lane of a gather on ONE table entry, a
                    broadcast: what the scan costs without LDS bank conflicts
  search            descriptors -> lists at every k, rerank = 0 and rerank = 4k (CUDA source), PQIndex and Int8Index
                    alternating (synchronised wall clock)
  recall@k          of PQIndex's raw and re-ranked lists against ranking.retrieve_device's lists (fp32 rows) and against
                    Int8Index's lists of the same rerank
Every timing is the median (min .. max) of `--repeats` after a warm-up.  The descriptors are scripts/bench_index.py's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import torch
from bench_index import alternating, descriptors, device_ms, recall, wall_ms
from dirtorch_amd import ops, ranking
from dirtorch_amd.index import Int8Index, PQIndex


def once_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def wall_alternating(fns, repeats):
    """bench_index.alternating on the synchronised wall clock, in seconds"""
    return alternating(fns, repeats, lambda fn: wall_ms(fn) / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', type=str, nargs='+', default=['70x1006322', '20000x20000'])
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--m', type=int, nargs='+', default=[64, 128])
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines, results = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    D = args.d
    centres = torch.randn(6, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    say('# product-quantised index beside the int8 index: D = %d; medians (min .. max) of %d timings after a warm-up' % (D, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    for shape in args.shapes:
        Q, N = (int(v) for v in shape.split('x'))
        b = descriptors(N, D, 6, centres)
        q = b if Q == N else descriptors(Q, D, 5, centres)
        same_set = Q == N
        flat = Int8Index(D).add(b)
        qc, qs = ops.quantize_rows(q)
        bytes8 = N * flat.codes.shape[1] + N * 4
        exact = {k: ranking.retrieve_device(q, b, k, same_set=same_set)[0] for k in args.k}
        for M in args.m:
            say('## Q = %d, N = %d, M = %d%s' % (Q, N, M, ' (the queries are the database: same_set)' if same_set else ''))
            res = {'q': Q, 'n': N, 'd': D, 'm': M}
            index = PQIndex(D, M)
            res['train_s'], _ = once_s(lambda: index.train(b))
            res['add_s'], _ = once_s(lambda: index.add(b))
            res['bytes_pq'], res['bytes_i8'] = index.nbytes(), bytes8
            say('bytes held: PQIndex %d (%d a row), Int8Index %d (%d a row + a 4-byte scale): %.4f of them; codes alone %d / %d = M / D'
                % (index.nbytes(), index.codes.shape[1], bytes8, flat.codes.shape[1], index.nbytes() / bytes8, M, D))
            say('PQIndex.train (%d rows sampled, 10 iterations) %8.3f s, PQIndex.add (%d rows) %8.3f s'
                % (min(N, 65536), res['train_s'], N, res['add_s']))
            chunk = int(max(1, min(Q, (1 << 30) // (4 * N + 1024 * M))))       # queries whose scores and tables fit 1 GiB
            lut = ops.pq_lut(q[:chunk], index.codebooks)
            out = torch.empty(chunk, N, dtype=torch.float32, device='cuda')
            equal = torch.zeros_like(index.codes)
            tl, = device_ms([lambda: ops.pq_lut(q[:chunk], index.codebooks)], args.inner, args.repeats)
            tp, t8, te = device_ms([lambda: ops.pq_scan(lut, index.codes, out=out),
                                    lambda: ops.similarity_i8(qc[:chunk], qs[:chunk], flat.codes, flat.scales, D, out=out),
                                    lambda: ops.pq_scan(lut, equal, out=out)], args.inner, args.repeats)
            looks = chunk * N * M
            res.update(scan_q=chunk, pq_lut_ms=tl[0], pq_scan_ms=tp[0], similarity_i8_ms=t8[0], pq_scan_equal_codes_ms=te[0])
            say('scan of %d queries: pq_lut   %8.3f ms (%.3f .. %.3f)' % (chunk, tl[0], tl[1], tl[2]))
            say('   pq_scan                  %8.3f ms (%.3f .. %.3f): %.3g look-ups = %.2f T look-ups/s; codes %.3f GB + scores %.3f GB'
                % (tp[0], tp[1], tp[2], looks, looks / tp[0] / 1e9, N * index.codes.shape[1] / 1e9, chunk * N * 4 / 1e9))
            say('   similarity_i8            %8.3f ms (%.3f .. %.3f): pq_scan / similarity_i8 = %.2f of the time'
                % (t8[0], t8[1], t8[2], tp[0] / t8[0]))
            say('   pq_scan, all codes equal %8.3f ms (%.3f .. %.3f): the same instructions, every gather a broadcast = %.2f of pq_scan'
                % (te[0], te[1], te[2], te[0] / tp[0]))
            del lut, out, equal
            res['search_s'], res['recall'] = {}, {}
            for k in args.k:
                for R in (0, 4 * k):
                    src = b if R else None
                    tq, ti = wall_alternating([lambda: index.search(q, k, rerank=R, source=src, same_set=same_set),
                                               lambda: flat.search(q, k, rerank=R, source=src, same_set=same_set)], args.repeats)
                    r_exact, r_i8, i8_exact = recall(tq[3][0], exact[k]), recall(tq[3][0], ti[3][0]), recall(ti[3][0], exact[k])
                    res['search_s']['%d/%d' % (k, R)] = [tq[0], ti[0]]
                    res['recall']['%d/%d' % (k, R)] = [r_exact, r_i8, i8_exact]
                    say('k = %4d rerank = %4d  PQIndex.search %8.4f s (%.4f .. %.4f)  Int8Index.search %8.4f s (%.4f .. %.4f);  recall@%d: '
                        'PQ vs fp32 lists %.4f, PQ vs Int8Index lists %.4f, Int8Index vs fp32 lists %.4f'
                        % (k, R, tq[0], tq[1], tq[2], ti[0], ti[1], ti[2], k, r_exact, r_i8, i8_exact))
            results.append(res)
            del index
        del flat, b, q, qc, qs, exact
        torch.cuda.empty_cache()
    print(json.dumps(results))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The inverted-file int8 index on one MI355X beside the flat int8 index it shortens, on bench_index.py's seeded descriptors.
    python scripts/bench_ivf.py [--q 70 1] [--n 1006322] [--d 2048] [--nlist 1024 4096] [--nprobe 1 8 32] [--k 10 100]
                                [--out profiles/ivf.txt]
  train / add          IVFInt8Index.train on the database itself (10 iterations) and add (synchronised wall clock, once)
  ivf_scan             dir_ivf_scan_i8 alone on prepared probe tables (the id pre-fill included), beside dir_similarity_i8 over
                       the whole database: device events, the two alternating inside every repeat; with the bytes each moves
  search               descriptors -> lists for every k, rerank = 0 and rerank = 4k (CUDA source): IVFInt8Index.search beside
                       Int8Index.search, alternating (synchronised wall clock)
  recall@k             share of the flat int8 lists' entries that the probed lists hold
Every point is the median (min .. max) of `--repeats` timings after a warm-up.  The database is bench_index.py's (`--clusters`
centres + noise, unit rows; 6 centres by default, where everything below the six clusters is noise: a hard case for any
inverted file - `--clusters 16384` gives every row about sixty relatives).  The queries are further rows of the SAME draw
(bench_index.descriptors hands a set of up to 2^17 rows to synth_descriptors, whose centres are its own: such queries are
unrelated to the database, which does not matter to a flat scan and makes recall meaningless here)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import torch
from bench_index import alternating, descriptors, event_ms, wall_ms
from dirtorch_amd import ops
from dirtorch_amd.index import IVFInt8Index, Int8Index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, nargs='+', default=[70, 1])
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--nlist', type=int, nargs='+', default=[1024, 4096])
    ap.add_argument('--nprobe', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--clusters', type=int, default=6)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    N, D = args.n, args.d
    assert N > 1 << 17, 'the device recipe of bench_index.descriptors starts above 2^17 rows'
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    b = descriptors(N + max(args.q), D, 6, centres, clusters=args.clusters)
    b, qall = b[:N], b[N:].clone()
    say('# inverted-file int8 index: N = %d, D = %d, %d cluster centres; medians (min .. max) of %d timings after a warm-up'
        % (N, D, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    flat = Int8Index(D).add(b)
    ldc = flat.codes.shape[1]
    result = {'n': N, 'd': D, 'points': []}
    for nlist in args.nlist:
        index = IVFInt8Index(D, nlist)
        t_train = wall_ms(lambda: index.train(b, iters=args.iters))
        t_add = wall_ms(lambda: index.add(b))
        lens = index._lens
        say('nlist = %d: train (%d iterations, %d rows) %.1f ms, add %.1f ms; list sizes %d .. %d, median %d'
            % (nlist, args.iters, min(N, 256 * nlist), t_train, t_add, lens.min(), lens.max(), int(statistics.median(lens.tolist()))))
        for Q in args.q:
            q = qall[:Q]
            qc, qs = ops.quantize_rows(q)
            flat_scores = torch.empty(Q, N, dtype=torch.float32, device='cuda')
            for nprobe in [p for p in args.nprobe if p <= nlist]:
                probe = index.probe(qc, qs, nprobe)
                plen = (index.list_off[1:] - index.list_off[:-1])[probe.long()]
                col_off = torch.cumsum(plen, dim=1, dtype=torch.int32) - plen
                tables = ops.ivf_probe_tables(index.list_off, probe, col_off)
                items, width = tables[4], tables[5]
                out = (torch.empty(Q, width, dtype=torch.float32, device='cuda'), torch.empty(Q, width, dtype=torch.int32, device='cuda'))
                # bytes: the codes of every (tile, group) once, the score and id of every candidate, the id pre-fill
                pairs = torch.bincount(probe.reshape(-1).long(), minlength=nlist).cpu().numpy()
                cand = int((pairs * lens).sum())
                scan_bytes = int((((pairs + 31) // 32) * lens).sum()) * ldc + cand * 8 + Q * width * 4
                flat_bytes = N * ldc + N * 4 + Q * N * 4
                ti, tf = alternating([lambda: ops.ivf_scan(qc, qs, index.codes, index.scales, index.ids, index.list_off, probe,
                                                           col_off, D, width=width, out=out, tables=tables),
                                      lambda: ops.similarity_i8(qc, qs, flat.codes, flat.scales, D, out=flat_scores)],
                                     args.repeats, lambda fn: event_ms(fn, args.inner))
                say('Q = %2d nlist = %4d nprobe = %2d  ivf_scan %8.4f ms (%.4f .. %.4f), %d workgroups, %.4f GB = %5.0f GB/s | flat '
                    'similarity_i8 %8.4f ms (%.4f .. %.4f), %.3f GB | %.3f of the flat time, %.4f of its bytes'
                    % (Q, nlist, nprobe, ti[0], ti[1], ti[2], items, scan_bytes / 1e9, scan_bytes / 1e6 / ti[0], tf[0], tf[1], tf[2],
                       flat_bytes / 1e9, ti[0] / tf[0], scan_bytes / flat_bytes))
                point = {'q': Q, 'nlist': nlist, 'nprobe': nprobe, 'ivf_scan_ms': ti[0], 'flat_scan_ms': tf[0], 'scan_bytes': scan_bytes,
                         'flat_bytes': flat_bytes, 'search_ms': {}, 'flat_search_ms': {}, 'recall': {}}
                for k in args.k:
                    for R in (0, 4 * k):
                        kw = dict(rerank=R, source=b if R else None)
                        si, sf = alternating([lambda: index.search(q, k, nprobe=nprobe, **kw), lambda: flat.search(q, k, **kw)],
                                             args.repeats, wall_ms)
                        got, want = si[3][0], sf[3][0]
                        hits = ((got.unsqueeze(2) == want.unsqueeze(1)) & (want.unsqueeze(1) >= 0)).any(dim=2).float().mean().item()
                        same = int((got == want).all(dim=1).sum())
                        say('    k = %3d rerank = %3d  IVFInt8Index.search %8.3f ms (%.3f .. %.3f) | Int8Index.search %8.3f ms (%.3f .. '
                            '%.3f) | %.3f of the flat time; recall@%d of the flat lists %.4f, %d of %d lists identical'
                            % (k, R, si[0], si[1], si[2], sf[0], sf[1], sf[2], si[0] / sf[0], k, hits, same, Q))
                        point['search_ms']['%d/%d' % (k, R)] = si[0]
                        point['flat_search_ms']['%d/%d' % (k, R)] = sf[0]
                        point['recall']['%d/%d' % (k, R)] = hits
                result['points'].append(point)
                del out
            del flat_scores
        del index
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

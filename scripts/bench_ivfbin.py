#!/usr/bin/env python
"""The inverted file over sign-bit rows on one MI355X beside the two other list scans and the flat binary scan, on
bench_index.py's seeded descriptors.
    python scripts/bench_ivfbin.py [--q 70] [--n 1006322] [--d 2048] [--nlist 1024] [--nprobe 1 8 32] [--search 8]
                                   [--k 10 100] [--rerank 2048] [--clusters 16384] [--out profiles/ivfbin.txt]
    python scripts/bench_ivfbin.py --all [--out profiles/ivfbin.txt]     the points of DESIGN.md 8.9, one child process each
  train / add    IVFInt8Index is trained on the database itself; IVFBinaryIndex and IVFFp4Index take its centroids and add
                 the same rows (synchronised wall clock, once); the three hold the same lists (asserted), so the probe
                 tables below are shared
  bytes          what IVFBinaryIndex, IVFFp4Index, IVFInt8Index and BinaryIndex hold on the device
  scan           dir_ivf_scan_bin (the query sums made before, as a search makes them once per chunk), dir_ivf_scan_fp4,
                 dir_ivf_scan_i8 over the SAME lists and probe tables (the id pre-fill included) and the flat
                 dir_similarity_bin over all rows: device events, the four alternating inside every repeat of one process
  search         at the --search values of nprobe: descriptors -> lists for every k, rerank = 0 and --rerank (CUDA source):
                 IVFBinaryIndex.search beside BinaryIndex.search and IVFFp4Index.search, alternating (synchronised wall
                 clock), and recall@k of each against ranking.retrieve_device's fp32 lists
Every point is the median (min .. max) of `--repeats` timings after a warm-up.  The queries are further rows of the
database's draw (bench_ivf.py).  --all runs every configuration in a fresh child process under a time limit of its own and
stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

# (flags, seconds): 70 queries and one query at 1 / 8 / 32 of 1024 lists on 16 384 centres (searches at 8), the six-centre
# data at 32 lists, 20 000 x 20 000 (lists of about 310 rows, and the 19-row lists of 1024; scans only)
POINTS = [(['--clusters', '16384', '--q', '70', '--nprobe', '1', '8', '32', '--search', '8'], 300),
          (['--clusters', '16384', '--q', '1', '--nprobe', '1', '8', '32', '--search'], 200),
          (['--clusters', '6', '--q', '70', '--nprobe', '32', '--search', '32'], 300),
          (['--clusters', '6', '--n', '20000', '--q', '20000', '--nlist', '64', '--nprobe', '8', '--search'], 200),
          (['--clusters', '6', '--n', '20000', '--q', '20000', '--nlist', '1024', '--nprobe', '8', '--search'], 200)]


def run_all(out):
    for flags, seconds in POINTS:
        cmd = [sys.executable, os.path.abspath(__file__)] + flags + (['--out', out] if out else [])
        print('+ ' + ' '.join(cmd[1:]), flush=True)
        rc = subprocess.run(cmd, timeout=seconds).returncode      # a child that overruns is killed and the run ends here
        if rc != 0:
            raise SystemExit('%s: exit status %d; the remaining points are not run' % (' '.join(flags), rc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--all', action='store_true')
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--nlist', type=int, default=1024)
    ap.add_argument('--nprobe', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--search', type=int, nargs='*', default=[8], help='the nprobe values at which the searches are timed too')
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--rerank', type=int, default=2048)
    ap.add_argument('--clusters', type=int, default=16384)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    if args.all:
        return run_all(args.out)
    import torch
    from bench_index import alternating, descriptors, event_ms, recall, wall_ms
    from dirtorch_amd import ops, ranking
    from dirtorch_amd.index import BinaryIndex, IVFBinaryIndex, IVFFp4Index, IVFInt8Index
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    Q, N, D, nlist = args.q, args.n, args.d, args.nlist
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    b = descriptors(N + Q, D, 6, centres, clusters=args.clusters)
    b, q = b[:N], b[N:].clone()
    say('# inverted file over sign-bit rows: Q = %d, N = %d, D = %d, nlist = %d, %d cluster centres; medians (min .. max) of %d '
        'timings after a warm-up' % (Q, N, D, nlist, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    result = {'q': Q, 'n': N, 'd': D, 'nlist': nlist, 'clusters': args.clusters, 'points': []}

    i8 = IVFInt8Index(D, nlist)
    IVFInt8Index(D, nlist).train(b, iters=1).add(b)       # warm-up at full size: kernels loaded, the allocator holds the big blocks
    t8 = wall_ms(lambda: i8.train(b, iters=args.iters))
    ib, i4 = IVFBinaryIndex(D, nlist), IVFFp4Index(D, nlist)
    for index in (ib, i4):                                # the same centroids: the same training, not timed three times
        index._set_centroids(i8.centroids.clone())
    for cls in (IVFBinaryIndex, IVFFp4Index):             # their adds warmed up too
        warm = cls(D, nlist)
        warm._set_centroids(i8.centroids.clone())
        warm.add(b)
        del warm
    ab, a4, a8 = wall_ms(lambda: ib.add(b)), wall_ms(lambda: i4.add(b)), wall_ms(lambda: i8.add(b))
    for other in (ib, i4):
        assert torch.equal(other.list_off, i8.list_off) and torch.equal(other.ids, i8.ids), 'the inverted files hold the same lists'
    flat = BinaryIndex(D).add(b)
    lens = i8._lens
    say('train (%d iterations, %d rows, IVFInt8Index; the others take its centroids): %.1f ms; add: IVFBinaryIndex %.1f ms, IVFFp4Index '
        '%.1f ms, IVFInt8Index %.1f ms; list sizes %d .. %d, median %d'
        % (args.iters, min(N, 256 * nlist), t8, ab, a4, a8, lens.min(), lens.max(), int(statistics.median(lens.tolist()))))
    ldc, lde = ops.fp4_widths(D)
    ld8, ldb = i8.codes.shape[1], ops.bin_width(D)
    bytes_i8 = i8.codes.numel() + 4 * i8.scales.numel() + 4 * i8.ids.numel()
    say('bytes held: IVFBinaryIndex %d (%d a row: %d bits + 4 + 4), IVFFp4Index %d (%d a row), IVFInt8Index %d (%d a row), BinaryIndex '
        '%d (%d a row)' % (ib.nbytes(), ldb + 8, ldb, i4.nbytes(), ldc + lde + 8, bytes_i8, ld8 + 8, flat.nbytes(), ldb + 4))
    result.update(train_ms=t8, add_ms=[ab, a4, a8], bytes=[ib.nbytes(), i4.nbytes(), bytes_i8, flat.nbytes()])

    c8, s8 = ops.quantize_rows(q)
    c4, e4, s4 = ops.quantize_rows_fp4(q)
    sums = ops.code_sums(c8, D)
    flat_out = torch.empty(Q, N, dtype=torch.float32, device='cuda')
    exact = {k: ranking.retrieve_device(q, b, k)[0] for k in args.k} if args.search else {}
    for nprobe in [p for p in args.nprobe if p <= nlist]:
        probe = i8.probe(c8, s8, nprobe)
        plen = (i8.list_off[1:] - i8.list_off[:-1])[probe.long()]
        col_off = torch.cumsum(plen, dim=1, dtype=torch.int32) - plen
        tables = ops.ivf_probe_tables(i8.list_off, probe, col_off)
        items, width = tables[4], tables[5]
        out = (torch.empty(Q, width, dtype=torch.float32, device='cuda'), torch.empty(Q, width, dtype=torch.int32, device='cuda'))
        # bytes: the rows of every (tile, group) once, the score and id of every candidate, the id pre-fill
        pairs = torch.bincount(probe.reshape(-1).long(), minlength=nlist).cpu().numpy()
        cand = int((pairs * lens).sum())
        reads = int((((pairs + 31) // 32) * lens).sum())
        moved = [reads * (w + 4) + cand * 8 + Q * width * 4 for w in (ldb, ldc + lde, ld8)]
        kw = dict(width=width, out=out, tables=tables)
        runs = alternating([lambda: ops.ivf_scan_bin(c8, s8, ib.codes, ib.scales, ib.ids, ib.list_off, probe, col_off, D, qsums=sums, **kw),
                            lambda: ops.ivf_scan_fp4(c4, e4, s4, i4.codes, i4.exps, i4.scales, i4.ids, i4.list_off, probe, col_off, D, **kw),
                            lambda: ops.ivf_scan(c8, s8, i8.codes, i8.scales, i8.ids, i8.list_off, probe, col_off, D, **kw),
                            lambda: ops.similarity_bin(c8, s8, flat.codes, flat.scales, D, out=flat_out)],
                           args.repeats, lambda fn: event_ms(fn, args.inner))
        tb, tf, ti, tl = [r[:3] for r in runs]
        best = min(tb[0], tf[0], ti[0])
        say('Q = %5d nprobe = %2d, %d workgroups, %d candidates  ivf_scan_bin %8.4f ms (%.4f .. %.4f), %.4f GB = %5.0f GB/s | ivf_scan_fp4 '
            '%8.4f ms (%.4f .. %.4f), %.4f GB | ivf_scan (int8) %8.4f ms (%.4f .. %.4f), %.4f GB | flat similarity_bin %8.4f ms (%.4f .. '
            '%.4f) | bin / fp4 %.3f, bin / int8 %.3f, bin / flat %.3f; the fastest list scan: %s'
            % (Q, nprobe, items, cand, tb[0], tb[1], tb[2], moved[0] / 1e9, moved[0] / 1e6 / tb[0], tf[0], tf[1], tf[2], moved[1] / 1e9,
               ti[0], ti[1], ti[2], moved[2] / 1e9, tl[0], tl[1], tl[2], tb[0] / tf[0], tb[0] / ti[0], tb[0] / tl[0],
               'bin' if best == tb[0] else 'fp4' if best == tf[0] else 'int8'))
        point = {'nprobe': nprobe, 'items': items, 'scan_bin_ms': tb[0], 'scan_fp4_ms': tf[0], 'scan_i8_ms': ti[0], 'flat_bin_ms': tl[0],
                 'bytes': moved, 'search_ms': {}, 'recall': {}}
        del out, runs
        for k in (args.k if nprobe in args.search else []):
            for R in (0, args.rerank):
                skw = dict(rerank=R, source=b if R else None)
                runs = alternating([lambda: ib.search(q, k, nprobe=nprobe, **skw), lambda: flat.search(q, k, **skw),
                                    lambda: i4.search(q, k, nprobe=nprobe, **skw)], args.repeats, wall_ms)
                names = ('IVFBinaryIndex', 'BinaryIndex', 'IVFFp4Index')
                hits = [recall(r[3][0], exact[k]) for r in runs]
                say('    k = %3d rerank = %4d  ' % (k, R) + ' | '.join('%s.search %8.3f ms (%.3f .. %.3f), recall@%d %.4f'
                                                                          % (n, r[0], r[1], r[2], k, h) for n, r, h in zip(names, runs, hits))
                    + ' | %.3f of the flat binary index\'s time, %.3f of the fp4 inverted file\'s'
                    % (runs[0][0] / runs[1][0], runs[0][0] / runs[2][0]))
                point['search_ms']['%d/%d' % (k, R)] = [r[0] for r in runs]
                point['recall']['%d/%d' % (k, R)] = hits
        result['points'].append(point)
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

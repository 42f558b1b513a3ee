#!/usr/bin/env python
"""The inverted file over fp4 codes on one MI355X beside the int8 inverted file and the flat fp4 index, on bench_index.py's
seeded descriptors.
    python scripts/bench_ivffp4.py [--q 70] [--n 1006322] [--d 2048] [--nlist 1024] [--nprobe 1 8 32] [--k 10 100]
                                   [--clusters 16384] [--out profiles/ivffp4.txt]
    python scripts/bench_ivffp4.py --all [--out profiles/ivffp4.txt]     the points of DESIGN.md 8.7, one child process each
  train / add    IVFFp4Index and IVFInt8Index on the database itself (synchronised wall clock, once); the two hold the same
                 lists (asserted), so the probe tables below are shared
  bytes          what IVFFp4Index, IVFInt8Index and Fp4Index hold on the device
  scan           dir_ivf_scan_fp4 beside dir_ivf_scan_i8 over the SAME lists and probe tables (the id pre-fill included):
                 device events, the two alternating inside every repeat of one process; with the bytes each moves
  search         descriptors -> lists for every k, rerank = 0 and rerank = 4k (CUDA source): IVFFp4Index.search beside
                 IVFInt8Index.search and Fp4Index.search, alternating (synchronised wall clock), and recall@k of each against
                 ranking.retrieve_device's fp32 lists
Every point is the median (min .. max) of `--repeats` timings after a warm-up.  The yardstick of a point is the int8 list
scan measured in the same process.  The queries are further rows of the database's draw (bench_ivf.py).  --all runs every
configuration in a fresh child process under a time limit of its own and stops at the first that fails."""
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

# (flags, seconds): 70 queries at 1 / 8 / 32 of 1024 lists and one query at 8 on 16 384 centres, the six-centre data at 32
# lists, 20 000 x 20 000 (lists of about 310 rows, and the 19-row lists of 1024)
POINTS = [(['--clusters', '16384', '--q', '70', '--nprobe', '1', '8', '32'], 300),
          (['--clusters', '16384', '--q', '1', '--nprobe', '8'], 300),
          (['--clusters', '6', '--q', '70', '--nprobe', '32'], 300),
          (['--clusters', '6', '--n', '20000', '--q', '20000', '--nlist', '64', '--nprobe', '8'], 300),
          (['--clusters', '6', '--n', '20000', '--q', '20000', '--nlist', '1024', '--nprobe', '8'], 300)]


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
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
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
    from dirtorch_amd.index import Fp4Index, IVFFp4Index, IVFInt8Index
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    Q, N, D, nlist = args.q, args.n, args.d, args.nlist
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    b = descriptors(N + Q, D, 6, centres, clusters=args.clusters)
    b, q = b[:N], b[N:].clone()
    say('# inverted file over fp4 codes: Q = %d, N = %d, D = %d, nlist = %d, %d cluster centres; medians (min .. max) of %d timings '
        'after a warm-up' % (Q, N, D, nlist, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    result = {'q': Q, 'n': N, 'd': D, 'nlist': nlist, 'clusters': args.clusters, 'points': []}

    i4, i8 = IVFFp4Index(D, nlist), IVFInt8Index(D, nlist)
    for cls in (IVFFp4Index, IVFInt8Index):       # warm-up at full size: kernels loaded, the allocator holds the big blocks
        cls(D, nlist).train(b, iters=1).add(b)
    t4, t8 = wall_ms(lambda: i4.train(b, iters=args.iters)), wall_ms(lambda: i8.train(b, iters=args.iters))
    a4, a8 = wall_ms(lambda: i4.add(b)), wall_ms(lambda: i8.add(b))
    assert torch.equal(i4.list_off, i8.list_off) and torch.equal(i4.ids, i8.ids), 'the two inverted files hold the same lists'
    flat = Fp4Index(D).add(b)
    lens = i4._lens
    say('train (%d iterations, %d rows): IVFFp4Index %.1f ms, IVFInt8Index %.1f ms; add: %.1f ms, %.1f ms; list sizes %d .. %d, median %d'
        % (args.iters, min(N, 256 * nlist), t4, t8, a4, a8, lens.min(), lens.max(), int(statistics.median(lens.tolist()))))
    ldc, lde = ops.fp4_widths(D)
    ld8 = i8.codes.shape[1]
    bytes_i8 = i8.codes.numel() + 4 * i8.scales.numel() + 4 * i8.ids.numel()
    say('bytes held: IVFFp4Index %d (%d a row: %d codes + %d block bytes + 4 + 4), IVFInt8Index %d (%d a row), Fp4Index %d (%d a row)'
        % (i4.nbytes(), ldc + lde + 8, ldc, lde, bytes_i8, ld8 + 8, flat.nbytes(), ldc + lde + 4))
    result.update(train_ms=[t4, t8], add_ms=[a4, a8], bytes=[i4.nbytes(), bytes_i8, flat.nbytes()])

    c8, s8 = ops.quantize_rows(q)
    c4, e4, s4 = ops.quantize_rows_fp4(q)
    exact = {k: ranking.retrieve_device(q, b, k)[0] for k in args.k}
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
        b4, b8 = reads * (ldc + lde + 4) + cand * 8 + Q * width * 4, reads * (ld8 + 4) + cand * 8 + Q * width * 4
        tf, ti = alternating([lambda: ops.ivf_scan_fp4(c4, e4, s4, i4.codes, i4.exps, i4.scales, i4.ids, i4.list_off, probe, col_off,
                                                       D, width=width, out=out, tables=tables),
                              lambda: ops.ivf_scan(c8, s8, i8.codes, i8.scales, i8.ids, i8.list_off, probe, col_off, D, width=width,
                                                   out=out, tables=tables)], args.repeats, lambda fn: event_ms(fn, args.inner))
        say('Q = %5d nprobe = %2d, %d workgroups, %d candidates  ivf_scan_fp4 %8.4f ms (%.4f .. %.4f), %.4f GB = %5.0f GB/s | ivf_scan '
            '(int8) %8.4f ms (%.4f .. %.4f), %.4f GB = %5.0f GB/s | %.3f of the int8 time, %.3f of its bytes; every fp4 timing below '
            'every int8 timing: %s' % (Q, nprobe, items, cand, tf[0], tf[1], tf[2], b4 / 1e9, b4 / 1e6 / tf[0], ti[0], ti[1], ti[2],
                                       b8 / 1e9, b8 / 1e6 / ti[0], tf[0] / ti[0], b4 / b8, tf[2] < ti[1]))
        point = {'nprobe': nprobe, 'items': items, 'scan_fp4_ms': tf[0], 'scan_i8_ms': ti[0], 'bytes_fp4': b4, 'bytes_i8': b8,
                 'search_ms': {}, 'recall': {}}
        del out
        for k in args.k:
            for R in (0, 4 * k):
                kw = dict(rerank=R, source=b if R else None)
                runs = alternating([lambda: i4.search(q, k, nprobe=nprobe, **kw), lambda: i8.search(q, k, nprobe=nprobe, **kw),
                                    lambda: flat.search(q, k, **kw)], args.repeats, wall_ms)
                names = ('IVFFp4Index', 'IVFInt8Index', 'Fp4Index')
                hits = [recall(r[3][0], exact[k]) for r in runs]
                say('    k = %3d rerank = %3d  ' % (k, R) + ' | '.join('%s.search %8.3f ms (%.3f .. %.3f), recall@%d %.4f'
                                                                         % (n, r[0], r[1], r[2], k, h) for n, r, h in zip(names, runs, hits))
                    + ' | %.3f of the int8 inverted file\'s time' % (runs[0][0] / runs[1][0]))
                point['search_ms']['%d/%d' % (k, R)] = [r[0] for r in runs]
                point['recall']['%d/%d' % (k, R)] = hits
        result['points'].append(point)
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""alpha-QE / DBA on one MI355X: the matrix route beside the list route, the self-set (DBA) on seeded unit-norm descriptors.
    python scripts/bench_expand.py [--n 20000] [--d 2048] [--k 10] [--alpha 3] [--matrix] [--out profiles/expand_lists.txt]
  matrix route      ops.expand_descriptors: the n x n fp32 score matrix in chunks and k selection rounds per row (only
                    with --matrix; at config D's size it is not run, its arithmetic is printed and marked as such)
  exact lists       ranking.retrieve_device(x, x, k, same_set=True), then ops.expand_lists
  index lists       IVFInt8Index(nlist).search(x, k, nprobe, rerank, same_set=True), then ops.expand_lists
  quality           the cosine between the rows of the exact-list and the index-list outputs
The routes alternate inside every repeat, in one process; every point is the median (min .. max) of `--repeats` timings
after a warm-up.  List-making and the matrix route are synchronised wall clocks (Python loops over chunks), the
expand_lists launch is timed by device events.  --no-exact leaves the exact lists out (and with them the quality figure).
The descriptors are scripts/bench_index.py's (tests/synth.py's recipe: cluster centres + noise, unit rows)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import torch
from bench_index import descriptors
from dirtorch_amd import ops, ranking
from dirtorch_amd.index import IVFInt8Index


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def fmt(ts):
    return '%10.3f ms (%.3f .. %.3f)' % (statistics.median(ts), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--alpha', type=float, default=3)
    ap.add_argument('--clusters', type=int, default=6)
    ap.add_argument('--nlist', type=int, default=0, help='0: 4 sqrt(n) rounded down to a power of two')
    ap.add_argument('--nprobe', type=int, default=8)
    ap.add_argument('--rerank', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--scratch-mb', type=int, default=256, help='scratch_bytes of the list makers (their default: 256)')
    ap.add_argument('--matrix', action='store_true', help='time ops.expand_descriptors too')
    ap.add_argument('--no-exact', action='store_true')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    N, D, k, alpha = args.n, args.d, args.k, args.alpha
    nlist = args.nlist or 1 << (int(4 * N ** 0.5).bit_length() - 1)
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    x = descriptors(N, D, 6, centres, clusters=args.clusters)
    say('# alpha-QE / DBA, self-set: N = %d, D = %d, k = %d, alpha = %g, %d cluster centres; medians (min .. max) of %d timings '
        'after a warm-up, the routes alternating inside every repeat; list makers with %d MiB of scratch' % (N, D, k, alpha, args.clusters, args.repeats, args.scratch_mb))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    t, index = wall(lambda: IVFInt8Index(D, nlist).train(x).add(x))
    say('IVFInt8Index(nlist = %d): train + add %.1f ms (once, not part of a route below)' % (nlist, t))
    scratch = args.scratch_mb << 20
    search = dict(nprobe=args.nprobe, rerank=args.rerank, source=x if args.rerank else None, scratch_bytes=scratch)
    routes = {'index lists': lambda: index.search(x, k, same_set=True, **search)}
    if not args.no_exact:
        routes['exact lists'] = lambda: ranking.retrieve_device(x, x, k, same_set=True, scratch_bytes=scratch)
    times = {name: ([], []) for name in routes}
    matrix_ms, outs = [], {}
    for rep in range(args.repeats + 1):      # (repeat 0 is the warm-up)
        if args.matrix:
            t, outs['matrix'] = wall(lambda: ops.expand_descriptors(x, None, alpha=alpha, k=k))
            if rep:
                matrix_ms.append(t)
        for name, make in routes.items():
            outs.pop(name, None)
            t_lists, (idx, vals) = wall(make)
            t_gather, outs[name] = event(lambda: ops.expand_lists(x, x, idx, vals, alpha))
            if rep:
                times[name][0].append(t_lists)
                times[name][1].append(t_gather)
            del idx, vals
        print('  repeat %d of %d done' % (rep, args.repeats), flush=True)
    moved = (k + 2) * N * 4 * D
    result = {'n': N, 'd': D, 'k': k, 'alpha': alpha, 'nlist': nlist, 'nprobe': args.nprobe, 'rerank': args.rerank}
    if args.matrix:
        say('matrix route   ops.expand_descriptors                       %s' % fmt(matrix_ms))
        result['matrix_ms'] = statistics.median(matrix_ms)
    else:
        say('matrix route   not run at this size.  ARITHMETIC, not a measurement: N^2 D = %.3g multiply-adds on the exact-fp32 '
            'MFMA path, then k N^2 = %.3g score reads (%.3g bytes) by the selection rounds' % (float(N) * N * D, float(k) * N * N,
                                                                                             4.0 * k * N * N))
    for name in routes:
        tl, tg = times[name]
        what = ('IVFInt8Index.search, nprobe = %d, rerank = %d' % (args.nprobe, args.rerank)) if name == 'index lists' \
            else 'ranking.retrieve_device'
        say('%s    %-45s %s' % (name, what, fmt(tl)))
        say('%s    ops.expand_lists (the gather)                 %s; it moves (k + 2) N 4D = %.3f GB = %.0f GB/s'
            % (' ' * len(name), fmt(tg), moved / 1e9, moved / 1e6 / statistics.median(tg)))
        say('%s    both                                          %10.3f ms' % (' ' * len(name), statistics.median(tl) + statistics.median(tg)))
        result[name.replace(' ', '_') + '_ms'] = [statistics.median(tl), statistics.median(tg)]
    if args.matrix and 'exact lists' in outs:
        cos = torch.nn.functional.cosine_similarity(outs['matrix'].double(), outs['exact lists'].double(), dim=1)
        say('matrix route against exact lists: 1 - cosine of the rows, largest %.3g (rows whose k-th neighbour is a near tie, '
            'or with fewer than k positive scores, may differ)' % float((1 - cos).max()))
    if len(routes) == 2:
        cos = torch.nn.functional.cosine_similarity(outs['exact lists'].double(), outs['index lists'].double(), dim=1)
        q = torch.quantile(cos, torch.tensor([0.01, 0.5], dtype=torch.float64, device=cos.device))
        say('quality: cosine between the exact-list and the index-list rows: mean %.6f, median %.6f, 1st percentile %.6f, '
            'smallest %.6f; %d of %d rows identical' % (float(cos.mean()), float(q[1]), float(q[0]), float(cos.min()),
                                                       int((outs['exact lists'] == outs['index lists']).all(dim=1).sum()), N))
        result['cosine_mean'], result['cosine_min'] = float(cos.mean()), float(cos.min())
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

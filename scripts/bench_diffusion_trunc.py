#!/usr/bin/env python
"""Truncated diffusion beside the full solve on one MI355X, the setting of scripts/bench_diffusion.py.
    python scripts/bench_diffusion_trunc.py [--n 20000] [--clusters 6] [--q 70] [--d 2048] [--k 50] [--kq 10] [--iters 20]
                                            [--trunc 256 1000 2048] [--out profiles/diffusion_trunc.txt]
The graph is made beforehand from IVFInt8Index lists (bench_diffusion.py's graph).  Per repeat, alternating in one process:
  full solve        ops.diffusion_seed + ops.diffusion_solve over all N rows: what diffuse_device costs online
  and for every T:
  subgraph          ops.diffusion_subgraph on candidate lists that are already there
  solve             ops.diffusion_solve_local, `iters` iterations, and one iteration as (t(iters) - t(iters / 2)) / (iters / 2)
  ranking           ops.topk(f, T, ids=cid)
  lists             ranking.diffuse_truncated_device(q, x, trunc=T, graph=..., index=...): descriptors to ranked lists, the
                    candidates from the IVFInt8Index (nprobe, rerank = T)
Single launches are timed by device events, the routes that loop in Python by synchronised wall clocks; every point is the
median (min .. max) of `--repeats` timings after a warm-up.  Quality: the share of the full diffusion's top 10 / top 100
that the truncated route's top 10 / top 100 hold, mean over the queries.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--kq', type=int, default=10)
    ap.add_argument('--gamma', type=float, default=3)
    ap.add_argument('--alpha', type=float, default=0.99)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--clusters', type=int, default=6)
    ap.add_argument('--nlist', type=int, default=0, help='0: 4 sqrt(n) rounded down to a power of two')
    ap.add_argument('--nprobe', type=int, default=8)
    ap.add_argument('--rerank', type=int, default=50, help='shortlist of the graph\'s index searches (>= k)')
    ap.add_argument('--trunc', type=int, nargs='+', default=[256, 1000, 2048])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    import torch
    from bench_index import descriptors
    from dirtorch_amd import ops, ranking
    from dirtorch_amd.index import IVFInt8Index
    assert torch.cuda.is_available(), 'a timing needs the GPU'

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
    N, Q, D, k, kq, iters = args.n, args.q, args.d, args.k, args.kq, args.iters
    half = max(1, iters // 2)
    nlist = args.nlist or 1 << (int(4 * N ** 0.5).bit_length() - 1)
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    both = descriptors(N + Q, D, 6, centres, clusters=args.clusters)      # one draw: the queries share the database's centres
    x, q = both[:N], both[N:]
    index = IVFInt8Index(D, nlist).train(x).add(x)
    lists = index.search(x, k, same_set=True, nprobe=args.nprobe, rerank=args.rerank, source=x)
    graph = (lists[0], ops.knn_graph(lists[0], lists[1], args.gamma))
    live = float((graph[1] != 0).float().sum(dim=1).mean())
    qidx, qvals = index.search(q, kq, nprobe=args.nprobe, rerank=args.rerank, source=x)
    truncs = [min(T, N, ops.diffusion_local_max_rows()) for T in args.trunc]
    cands = {T: index.search(q, T, nprobe=args.nprobe, rerank=T, source=x) for T in truncs}
    say('# truncated diffusion: N = %d, Q = %d, D = %d, k = %d, kq = %d, gamma = %g, alpha = %g, iters = %d, %d cluster centres, '
        'IVFInt8Index(nlist = %d) nprobe = %d; the graph keeps %.1f of %d slots per row; medians (min .. max) of %d timings after a '
        'warm-up, the routes alternating inside every repeat' % (N, Q, D, k, kq, args.gamma, args.alpha, iters, args.clusters, nlist,
                                                                   args.nprobe, live, k, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    times, outs = {}, {}
    dk = dict(gamma=args.gamma, alpha=args.alpha, iters=iters)

    def full():
        Y = ops.diffusion_seed(qidx, qvals, N, args.gamma)
        return ops.diffusion_solve(graph[0], graph[1], Y, alpha=args.alpha, iters=iters)
    for rep in range(args.repeats + 1):      # (repeat 0 is the warm-up)
        runs = [('full', event, full),
                ('full_online', wall, lambda: ranking.diffuse_device(q, x, k=k, kq=kq, graph=graph, index=index, nprobe=args.nprobe,
                                                                     rerank=args.rerank, **dk))]
        for T in truncs:
            ci, cv = cands[T]
            sub = ops.diffusion_subgraph(graph[0], graph[1], ci, cv, kq=kq, gamma=args.gamma)
            cid, lidx, lw, y = sub
            f = ops.diffusion_solve_local(lidx, lw, y, cid=cid, alpha=args.alpha, iters=iters)
            runs += [(('subgraph', T), event, lambda ci=ci, cv=cv: ops.diffusion_subgraph(graph[0], graph[1], ci, cv, kq=kq, gamma=args.gamma)),
                     (('solve', T), event, lambda s=sub: ops.diffusion_solve_local(s[1], s[2], s[3], cid=s[0], alpha=args.alpha, iters=iters)),
                     (('half', T), event, lambda s=sub: ops.diffusion_solve_local(s[1], s[2], s[3], cid=s[0], alpha=args.alpha, iters=half)),
                     (('rank', T), event, lambda f=f, cid=cid, T=T: ops.topk(f, T, ids=cid)),
                     (('lists', T), wall, lambda T=T: ranking.diffuse_truncated_device(
                         q, x, trunc=T, k=k, kq=kq, graph=graph, index=index, nprobe=args.nprobe, rerank=T, **dk))]
        for name, clock, fn in runs:
            outs.pop(name, None)
            t, outs[name] = clock(fn)
            if rep:
                times.setdefault(name, []).append(t)
        print('  repeat %d of %d done' % (rep, args.repeats), flush=True)
    med = {name: statistics.median(ts) for name, ts in times.items()}
    say('full solve     ops.diffusion_seed + ops.diffusion_solve, all %d rows, %d iterations   %s' % (N, iters, fmt(times['full'])))
    say('full online    diffuse_device(graph=...), the same index                              %s' % fmt(times['full_online']))
    top_full = ops.topk(outs['full'].t().contiguous(), 100)[0]
    result = {'n': N, 'q': Q, 'k': k, 'iters': iters, 'live': live, 'full_solve_ms': med['full'], 'full_online_ms': med['full_online']}
    for T in truncs:
        per = (med['solve', T] - med['half', T]) / (iters - half) if iters > half else float('nan')
        edges = float((outs['subgraph', T][1] >= 0).float().sum(dim=1).mean())      # live local slots per local row
        say('T = %-4d       subgraph %s   solve %s   ranking %s' % (T, fmt(times['subgraph', T]), fmt(times['solve', T]),
                                                                    fmt(times['rank', T])))
        say('               one iteration, (t(%d) - t(%d)) / %d = %.2f us for %d queries; a workgroup reads T k 8 B = %.0f KB of its '
            'local graph per iteration (%.1f of %d local slots per row are live), %.3f GB in all = %.0f GB/s; the three steps '
            'together %.3f ms against %.3f ms of the full solve (%.1f x)'
            % (iters, half, iters - half, per * 1e3, Q, T * k * 8 / 1e3, edges, k, Q * T * k * 8 / 1e9,
               Q * T * k * 8 / 1e6 / per if per > 0 else float('nan'),
               med['subgraph', T] + med['solve', T] + med['rank', T], med['full'],
               med['full'] / (med['subgraph', T] + med['solve', T] + med['rank', T])))
        say('               descriptors to lists, diffuse_truncated_device(graph=..., index, rerank = %d)   %s' % (T, fmt(times['lists', T])))
        got = outs['lists', T][0]
        shares = []
        for top in (10, 100):
            top = min(top, T)
            hit = (top_full[:, :top].unsqueeze(2) == got[:, :top].unsqueeze(1)).any(dim=2).float().mean()
            shares.append((top, 100 * float(hit)))
        say('               quality: its top %d holds %.1f %% of the full diffusion\'s top %d, its top %d %.1f %% of the top %d'
            % (shares[0][0], shares[0][1], shares[0][0], shares[1][0], shares[1][1], shares[1][0]))
        result['T%d' % T] = {'subgraph_ms': med['subgraph', T], 'solve_ms': med['solve', T], 'rank_ms': med['rank', T],
                             'iteration_us': per * 1e3, 'lists_ms': med['lists', T], 'top10': shares[0][1], 'top100': shares[1][1]}
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

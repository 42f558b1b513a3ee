#!/usr/bin/env python
"""Diffusion re-ranking on one MI355X: graph build, solve and the whole route, beside the host route a user would write.
    python scripts/bench_diffusion.py [--n 20000] [--q 70] [--d 2048] [--k 50] [--kq 10] [--iters 20] [--out profiles/diffusion.txt]
  graph build       ops.knn_graph on self-set lists that are already there (device events)
  solve             ops.diffusion_solve, `iters` iterations, and one iteration as (t(iters) - t(iters / 2)) / (iters / 2)
  exact lists       ranking.diffuse_device(q, x): retrieve_device lists for the graph and the queries, seeds, solve, transpose
  index lists       the same with index=IVFInt8Index(nlist), nprobe, rerank
  online            ranking.diffuse_device(q, x, graph=...) with the graph made beforehand: what a query batch costs
  host baseline     the same graph as a scipy.sparse CSR matrix and scipy.sparse.linalg.cg per query (maxiter = iters; rtol
                    1e-12, so a column whose residual has vanished stops early: nothing else guards scipy's 0 / 0 in fp32) on `--threads` threads; torch CPU sparse with the same CG loop where scipy is missing
The routes alternate inside every repeat, in one process; every point is the median (min .. max) of `--repeats` timings
after a warm-up (`--exact-repeats` for the exact lists, which take half a minute at 10^6 rows).  Routes that loop in Python
are synchronised wall clocks, single launches are timed by device events.
The apply kernel's own time comes from a kernel trace, taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_diffusion.py --n N --trace
    python scripts/bench_diffusion.py --n N --kernel-stats DIR [--out ...]
--trace runs ten solves on index lists and times nothing; --kernel-stats reads the rocpd database under DIR and prints
every diffusion kernel's average with the bytes the apply step moves, (k + 2) N 4 Qp for the vectors + 8 k N for the lists.
The descriptors are scripts/bench_index.py's (tests/synth.py's recipe: cluster centres + noise, unit rows)."""
import argparse
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def apply_bytes(N, Q, k):
    qp = (Q + 3) // 4 * 4
    return (k + 2) * N * 4 * qp + 8 * k * N


def kernel_stats(args, say):
    """the diffusion kernels of a rocprofv3 --kernel-trace --stats run: the `kernels` view of its rocpd database"""
    import sqlite3
    from collections import defaultdict
    files = glob.glob(os.path.join(args.kernel_stats, '**', '*.db'), recursive=True)
    assert files, 'no rocprofv3 .db under ' + args.kernel_stats
    agg = defaultdict(list)
    for name, dur in sqlite3.connect(files[0]).execute('select name, duration from kernels'):
        if 'diffusion_' in name or 'knn_' in name:
            agg[name.split('(')[0].replace('dir::', '').replace('void ', '')].append(dur / 1e3)
    say('# kernel trace (rocprofv3 --kernel-trace --stats, a run of its own: ten solves of %d iterations, N = %d, Q = %d, '
        'k = %d, index lists)' % (args.iters, args.n, args.q, args.k))
    for name, us in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        line = '%-34s %6d calls, average %9.1f us, median %9.1f us' % (name[:34], len(us), sum(us) / len(us), statistics.median(us))
        if 'diffusion_apply_kernel' in name:
            moved = apply_bytes(args.n, args.q, args.k)
            line += '; (k + 2) N 4 Qp + 8 k N = %.3f GB would be %.0f GB/s' % (moved / 1e9, moved / 1e3 / statistics.median(us))
            if args.live:
                real = (args.live + 2) * args.n * 4 * ((args.q + 3) // 4 * 4) + 8 * args.k * args.n
                line += '; with %.1f live slots per row it moves %.3f GB = %.0f GB/s' % (args.live, real / 1e9,
                                                                                         real / 1e3 / statistics.median(us))
        say(line)


def host_solve(idx, S, Y, alpha, iters, threads):
    """(F [N,Q], seconds to build the matrix, seconds to solve): CSR + scipy cg per query on a thread pool, or torch"""
    import numpy as np
    N, k = idx.shape
    t0 = time.perf_counter()
    live = (S != 0) & (idx >= 0) & (idx < N)
    rows = np.repeat(np.arange(N), k)[live.ravel()]
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import cg
        from concurrent.futures import ThreadPoolExecutor
        A = sp.identity(N, dtype=np.float32, format='csr') - np.float32(alpha) * sp.csr_matrix(
            (S.ravel()[live.ravel()], (rows, idx.ravel()[live.ravel()])), shape=(N, N), dtype=np.float32)
        t1 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            cols = list(pool.map(lambda c: cg(A, Y[:, c], rtol=1e-12, atol=0.0, maxiter=iters)[0], range(Y.shape[1])))
        return np.stack(cols, axis=1), t1 - t0, time.perf_counter() - t1, 'scipy.sparse CSR + scipy.sparse.linalg.cg per query'
    except ImportError:
        import torch
        torch.set_num_threads(threads)
        Sm = torch.sparse_coo_tensor(np.stack([rows, idx.ravel()[live.ravel()]]), S.ravel()[live.ravel()], (N, N)).to_sparse_csr()
        t1 = time.perf_counter()
        y = torch.from_numpy(Y)
        x, r, p = torch.zeros_like(y), y.clone(), y.clone()
        rr = (r * r).sum(0)
        for _ in range(iters):
            ap = p - alpha * (Sm @ p)
            pap = (p * ap).sum(0)
            a = torch.where(pap > 0, rr / pap, torch.zeros_like(pap))
            x, r = x + a * p, r - a * ap
            rn = (r * r).sum(0)
            p = r + torch.where(rr > 0, rn / rr, torch.zeros_like(rr)) * p
            rr = rn
        return x.numpy(), t1 - t0, time.perf_counter() - t1, 'torch CPU sparse CSR, the same CG loop on all columns'


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
    ap.add_argument('--rerank', type=int, default=50, help='shortlist of the index searches (>= k)')
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--exact-repeats', type=int, default=0, help='repeats of the exact-list route (0: --repeats)')
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--no-exact', action='store_true')
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--trace', action='store_true', help='ten solves on index lists for a kernel trace, nothing timed')
    ap.add_argument('--kernel-stats', type=str, default='', help='directory of a rocprofv3 --kernel-trace --stats run')
    ap.add_argument('--live', type=float, default=0, help='with --kernel-stats: live slots per row of the traced graph')
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush_out():
        if args.out:
            with open(args.out, 'a') as f:
                f.write('\n'.join(lines) + '\n\n')
    if args.kernel_stats:
        kernel_stats(args, say)
        flush_out()
        return
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
    N, Q, D, k, kq = args.n, args.q, args.d, args.k, args.kq
    dk = dict(gamma=args.gamma, alpha=args.alpha, iters=args.iters)
    nlist = args.nlist or 1 << (int(4 * N ** 0.5).bit_length() - 1)
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    both = descriptors(N + Q, D, 6, centres, clusters=args.clusters)      # one draw: the queries share the database's centres
    x, q = both[:N], both[N:]
    t, index = wall(lambda: IVFInt8Index(D, nlist).train(x).add(x))
    by_index = dict(index=index, nprobe=args.nprobe, rerank=args.rerank)
    if args.trace:
        graph = ranking.knn_graph_device(x, k, args.gamma, **by_index)
        qidx, qvals = index.search(q, kq, nprobe=args.nprobe, rerank=args.rerank, source=x)
        Y = ops.diffusion_seed(qidx, qvals, N, args.gamma)
        for _ in range(10):
            ops.diffusion_solve(graph[0], graph[1], Y, alpha=args.alpha, iters=args.iters)
        torch.cuda.synchronize()
        return
    say('# diffusion re-ranking: N = %d, Q = %d, D = %d, k = %d, kq = %d, gamma = %g, alpha = %g, iters = %d, %d cluster centres; '
        'medians (min .. max) of %d timings after a warm-up, the routes alternating inside every repeat'
        % (N, Q, D, k, kq, args.gamma, args.alpha, args.iters, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    say('IVFInt8Index(nlist = %d): train + add %.1f ms (once, not part of a route below)' % (nlist, t))
    exact_repeats = 0 if args.no_exact else (args.exact_repeats or args.repeats)
    lists_i = index.search(x, k, same_set=True, nprobe=args.nprobe, rerank=args.rerank, source=x)
    graph_i = (lists_i[0], ops.knn_graph(lists_i[0], lists_i[1], args.gamma))
    qidx, qvals = index.search(q, kq, nprobe=args.nprobe, rerank=args.rerank, source=x)
    Y = ops.diffusion_seed(qidx, qvals, N, args.gamma)
    half = max(1, args.iters // 2)
    T = {name: [] for name in ('graph', 'solve', 'half', 'index', 'online', 'exact')}
    outs = {}
    for rep in range(args.repeats + 1):      # (repeat 0 is the warm-up)
        runs = [('graph', event, lambda: ops.knn_graph(lists_i[0], lists_i[1], args.gamma)),
                ('solve', event, lambda: ops.diffusion_solve(graph_i[0], graph_i[1], Y, alpha=args.alpha, iters=args.iters)),
                ('half', event, lambda: ops.diffusion_solve(graph_i[0], graph_i[1], Y, alpha=args.alpha, iters=half)),
                ('index', wall, lambda: ranking.diffuse_device(q, x, k=k, kq=kq, **dk, **by_index)),
                ('online', wall, lambda: ranking.diffuse_device(q, x, k=k, kq=kq, graph=graph_i, **dk, **by_index))]
        if rep <= exact_repeats and exact_repeats:
            runs.append(('exact', wall, lambda: ranking.diffuse_device(q, x, k=k, kq=kq, **dk)))
        for name, clock, fn in runs:
            outs.pop(name, None)
            t, outs[name] = clock(fn)
            if rep:
                T[name].append(t)
        print('  repeat %d of %d done' % (rep, args.repeats), flush=True)
    live = float((graph_i[1] != 0).float().sum(dim=1).mean())
    unusable = int(((lists_i[0] < 0) | ~(lists_i[1] > 0)).sum())
    say('graph build    ops.knn_graph (index lists in place)            %s; %.1f of %d slots per row keep a mutual edge '
        '(%d of the %d list slots are empty or carry no positive score; the graph is %s)'
        % (fmt(T['graph']), live, k, unusable, N * k, 'finite' if bool(torch.isfinite(graph_i[1]).all()) else 'NOT finite'))
    say('solve          ops.diffusion_solve, %2d iterations              %s' % (args.iters, fmt(T['solve'])))
    per = (statistics.median(T['solve']) - statistics.median(T['half'])) / (args.iters - half) if args.iters > half else float('nan')
    moved = apply_bytes(N, Q, k)
    moved_live = int((live + 2) * N * 4 * ((Q + 3) // 4 * 4) + 8 * k * N)
    say('               one iteration, (t(%d) - t(%d)) / %d             %10.3f ms: apply, two column passes, x / r and p updates; '
        'the apply step alone moves (k + 2) N 4 Qp + 8 k N = %.3f GB if every slot is live, (%.1f + 2) N 4 Qp + 8 k N = %.3f GB '
        'on this graph (a dead slot re-reads the lane\'s own row); its own time: the kernel trace'
        % (args.iters, half, args.iters - half, per, moved / 1e9, live, moved_live / 1e9))
    say('index lists    diffuse_device, IVFInt8Index nprobe = %d, rerank = %d %s' % (args.nprobe, args.rerank, fmt(T['index'])))
    say('online         diffuse_device(graph=...), the same index        %s' % fmt(T['online']))
    result = {'n': N, 'q': Q, 'd': D, 'k': k, 'kq': kq, 'iters': args.iters, 'live': live, 'graph_ms': statistics.median(T['graph']),
              'solve_ms': statistics.median(T['solve']), 'iteration_ms': per, 'index_ms': statistics.median(T['index']),
              'online_ms': statistics.median(T['online'])}
    if exact_repeats:
        say('exact lists    diffuse_device, retrieve_device lists (%d timings) %s' % (len(T['exact']), fmt(T['exact'])))
        result['exact_ms'] = statistics.median(T['exact'])
        top = 10
        a, b = ops.topk(outs['exact'], top)[0], ops.topk(outs['index'], top)[0]
        same = (a.unsqueeze(2) == b.unsqueeze(1)).any(dim=2).float().mean()
        say('quality: the top %d of the index-list route holds %.1f %% of the top %d of the exact-list route' % (top, 100 * float(same), top))
    if not args.no_host:
        idx_h, S_h, Y_h = graph_i[0].cpu().numpy(), graph_i[1].cpu().numpy(), Y.cpu().numpy()
        tb, ts = [], []
        for _ in range(args.host_repeats):
            F_h, t_build, t_solve, what = host_solve(idx_h, S_h, Y_h, args.alpha, args.iters, args.threads)
            tb.append(t_build * 1e3)
            ts.append(t_solve * 1e3)
        F_d = ops.diffusion_solve(graph_i[0], graph_i[1], Y, alpha=args.alpha, iters=args.iters).cpu().numpy()
        scale = float(abs(F_h).max())
        say('host baseline  %s, %d threads, %d timings: matrix %s, solve %s' % (what, args.threads, len(ts), fmt(tb), fmt(ts)))
        say('               device solve against it: max |difference| / max |f| = %.3g' % (float(abs(F_d - F_h).max()) / scale))
        result['host_build_ms'], result['host_solve_ms'] = statistics.median(tb), statistics.median(ts)
    print(json.dumps(result))
    flush_out()


if __name__ == '__main__':
    main()

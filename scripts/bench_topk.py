#!/usr/bin/env python
"""Ranked neighbour lists on one MI355X: the device route against the route it replaces, on seeded unit-norm descriptors.
    python scripts/bench_topk.py [--q 70] [--n 1006322] [--d 2048] [--k 10 100 1024] [--out profiles/topk.txt]
  ops.topk          dir_topk alone on the Q x N score matrix (device events around `--inner` calls; the workspace
                    allocation of the wrapper is inside), beside ops.rank_counts on the same scores with the list's own k
                    indices as probes: both read every score once
  retrieve_device   descriptors on the device -> lists on the device (similarity + dir_topk per chunk of query rows),
                    a synchronised wall clock
  host route        ranking.similarity_device(...).cpu(), then np.argsort(kind='stable')[::-1][:, :k] over the rows on
                    `--threads` threads (numpy sorts outside the GIL); the sort does not depend on k, so it is timed once
Every point is the median of `--repeats` timings after a warm-up call.  ops.topk's lists are compared with the host route's
(same score matrix: they must be identical), retrieve_device's are compared too (its chunks are scored apart, so a score's
last bits - and with them two near-equal neighbours - may differ; see ranking.eval_labelled_device)."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
import numpy as np
import torch
from dirtorch_amd import ops, ranking


def descriptors(rows, d, seed, chunk=65536):
    """[rows, d] fp32 unit-norm rows on the device, drawn in chunks (8 GB at config D's database)."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    out = torch.empty(rows, d, dtype=torch.float32, device='cuda')
    centre = torch.randn(d, generator=g, device='cuda')
    for r0 in range(0, rows, chunk):
        x = torch.randn(min(chunk, rows - r0), d, generator=g, device='cuda') + 0.3 * centre
        out[r0:r0 + chunk] = torch.nn.functional.normalize(x, dim=1)
    return out


def device_ms(fn, inner, repeats):
    """Median, min, max over `repeats` event timings of `inner` back-to-back calls, per call, after a warm-up."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return statistics.median(ts), min(ts), max(ts)


def wall_s(fn, repeats, warm=True):
    if warm:
        fn()
    ts = []
    out = None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def host_route(q, b, kmax, pool):
    scores = ranking.similarity_device(q, b).cpu().numpy()
    order = list(pool.map(lambda row: np.argsort(row, kind='stable')[::-1][:kmax], scores))
    return np.stack(order), scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100, 1024])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    Q, N, D = args.q, args.n, args.d
    b = descriptors(N, D, 5)
    q = descriptors(Q, D, 6)
    say('# ranked neighbour lists: Q = %d, N = %d, D = %d; medians (min .. max) of %d timings after a warm-up'
        % (Q, N, D, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    scores = ranking.similarity_device(q, b)
    torch.cuda.synchronize()
    row_mb = Q * N * 4 / 1e6
    result = {'q': Q, 'n': N, 'd': D, 'topk_ms': {}, 'rank_counts_ms': {}, 'retrieve_s': {}}
    lists = {}
    for k in args.k:
        idx, _ = ops.topk(scores, k)
        lists[k] = idx.cpu().numpy()
        probes = torch.where(idx >= 0, idx, torch.zeros_like(idx)).contiguous()
        t = device_ms(lambda: ops.topk(scores, k), args.inner, args.repeats)
        c = device_ms(lambda: ops.rank_counts(scores, probes), args.inner, args.repeats)
        result['topk_ms'][k], result['rank_counts_ms'][k] = t[0], c[0]
        say('k = %4d  ops.topk %8.3f ms (%.3f .. %.3f) = %6.0f GB/s of score reads;  ops.rank_counts, %d probes per query, %8.3f ms '
            '(%.3f .. %.3f) = %6.0f GB/s' % (k, t[0], t[1], t[2], row_mb / t[0], k, c[0], c[1], c[2], row_mb / c[0]))
    del scores
    got = {}
    for k in args.k:
        t = wall_s(lambda: ranking.retrieve_device(q, b, k), args.repeats)
        result['retrieve_s'][k] = t[0]
        got[k] = t[3][0].cpu().numpy()
        say('k = %4d  retrieve_device, descriptors -> lists on the device: %8.4f s (%.4f .. %.4f)' % (k, t[0], t[1], t[2]))
    kmax = max(args.k)
    with ThreadPoolExecutor(args.threads) as pool:
        t = wall_s(lambda: host_route(q, b, kmax, pool), args.host_repeats, warm=False)
    result['host_s'] = t[0]
    say('host route, any k <= %d: similarity_device(...).cpu() + np.argsort(kind=\'stable\')[::-1][:, :k] on %d threads: %8.3f s '
        '(%.3f .. %.3f), %d repeats, the first counted' % (kmax, args.threads, t[0], t[1], t[2], args.host_repeats))
    order = t[3][0]
    for k in args.k:
        want = order[:, :k]
        say('k = %4d  ops.topk lists == host lists: %s;  retrieve_device lists == host lists in %d of %d queries;  speed-up of '
            'retrieve_device over the host route %.0fx' % (k, bool((lists[k] == want).all()), int((got[k] == want).all(axis=1).sum()), Q,
                                                        t[0] / result['retrieve_s'][k]))
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

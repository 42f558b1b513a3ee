#!/usr/bin/env python
"""The int8 descriptor index on one MI355X, beside the fp32 route it shortens, on seeded unit-norm descriptors.
    python scripts/bench_index.py [--q 70] [--n 1006322] [--d 2048] [--k 10 100] [--out profiles/index_i8.txt]
  quantize_rows     dir_quantize_rows_i8 over the whole database (device events)
  similarity_i8     the scan alone, beside ops.similarity(unit_range=True) on the fp32 rows: same process, the two
                    alternating inside every repeat, both writing the same Q x N fp32 scores
  Int8Index.search  descriptors -> lists, rerank = 0 and rerank = 4k (CUDA source), beside ranking.retrieve_device
                    (synchronised wall clock)
  agreement         share of the queries whose list equals retrieve_device's list, and recall@k of the raw scan
Every point is the median (min .. max) of `--repeats` timings after a warm-up.  The descriptors follow
tests/synth.py:synth_descriptors (six cluster centres + noise, unit rows): up to 2^17 rows they ARE synth_descriptors,
above that they are drawn on the device in chunks with the same recipe (the numpy generator would need 48 GB of host
memory at 10^6 x 2048)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch
from dirtorch_amd import ops, ranking
from dirtorch_amd.index import Int8Index


def descriptors(rows, d, seed, centres, chunk=65536, clusters=6, noise=0.35):
    if rows <= 1 << 17:
        from synth import synth_descriptors
        return torch.from_numpy(synth_descriptors(seed, rows, d, clusters, noise)).cuda()
    g = torch.Generator(device='cuda').manual_seed(seed)
    out = torch.empty(rows, d, dtype=torch.float32, device='cuda')
    for r0 in range(0, rows, chunk):
        n = min(chunk, rows - r0)
        pick = torch.randint(0, clusters, (n,), generator=g, device='cuda')
        x = centres[pick] + 3.0 * noise * torch.randn(n, d, generator=g, device='cuda')
        out[r0:r0 + n] = torch.nn.functional.normalize(x, dim=1)
    return out


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(fns, repeats, timer):
    """[(median, min, max, the result of the warm-up call)] per function over `repeats` timings; the functions alternate inside a repeat"""
    outs = [fn() for fn in fns]
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            ts[i].append(timer(fn))
    return [(statistics.median(t), min(t), max(t), o) for t, o in zip(ts, outs)]


def device_ms(fns, inner, repeats):
    """[(median, min, max)] per function over `repeats` event timings of `inner` calls; the functions alternate."""
    return [t[:3] for t in alternating(fns, repeats, lambda fn: event_ms(fn, inner))]


def recall(got, ref):
    """the share of ref's list entries that got's list of the same query holds, in chunks of queries"""
    hits, rows = 0, max(1, (1 << 26) // (got.shape[1] * ref.shape[1]))
    for r0 in range(0, got.shape[0], rows):
        g, e = got[r0:r0 + rows], ref[r0:r0 + rows]
        hits += int(((g.unsqueeze(2) == e.unsqueeze(1)) & (e.unsqueeze(1) >= 0)).any(dim=1).sum())
    return hits / max(float((ref >= 0).sum()), 1.0)


def wall_s(fn, repeats):
    fn()
    ts, out = [], None
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    Q, N, D = args.q, args.n, args.d
    centres = torch.randn(6, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    b = descriptors(N, D, 6, centres)
    q = descriptors(Q, D, 5, centres)
    say('# int8 descriptor index: Q = %d, N = %d, D = %d; medians (min .. max) of %d timings after a warm-up' % (Q, N, D, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    result = {'q': Q, 'n': N, 'd': D}

    t, = device_ms([lambda: ops.quantize_rows(b)], args.inner, args.repeats)
    gb = N * D * 5 / 1e9
    result['quantize_ms'] = t[0]
    say('quantize_rows, %d rows: %8.3f ms (%.3f .. %.3f) = %5.0f GB/s of fp32 read + codes written' % (N, t[0], t[1], t[2], gb / t[0] * 1e3))

    index = Int8Index(D).add(b)
    qc, qs = ops.quantize_rows(q)
    out8 = torch.empty(Q, N, dtype=torch.float32, device='cuda')
    t8, tp = device_ms([lambda: ops.similarity_i8(qc, qs, index.codes, index.scales, D, out=out8),
                        lambda: ops.similarity(q, b, unit_range=True)], args.inner, args.repeats)
    bytes8 = N * index.codes.shape[1] + N * 4 + Q * N * 4
    bytesp = N * D * 4 + Q * N * 4
    result.update(similarity_i8_ms=t8[0], similarity_pair_ms=tp[0])
    say('similarity_i8                 %8.3f ms (%.3f .. %.3f): %.2f GB (codes once + scores) = %5.0f GB/s'
        % (t8[0], t8[1], t8[2], bytes8 / 1e9, bytes8 / 1e6 / t8[0]))
    say('ops.similarity(unit_range)    %8.3f ms (%.3f .. %.3f): %.2f GB (fp32 rows once + scores) = %5.0f GB/s'
        % (tp[0], tp[1], tp[2], bytesp / 1e9, bytesp / 1e6 / tp[0]))
    faster = t8[2] < tp[1]
    say('int8 scan / fp32 scan = %.3f of the time (%.2fx); every int8 timing below every fp32 timing: %s'
        % (t8[0] / tp[0], tp[0] / t8[0], faster))
    result['scan_faster_beyond_spread'] = bool(faster)
    del out8

    result['search_s'], result['retrieve_s'], result['agreement'] = {}, {}, {}
    for k in args.k:
        tr = wall_s(lambda: ranking.retrieve_device(q, b, k), args.repeats)
        exact = tr[3][0]
        result['retrieve_s'][k] = tr[0]
        say('k = %4d  retrieve_device (fp32 rows)              %8.4f s (%.4f .. %.4f)' % (k, tr[0], tr[1], tr[2]))
        for R in (0, 4 * k):
            ts = wall_s(lambda: index.search(q, k, rerank=R, source=b if R else None), args.repeats)
            got = ts[3][0]
            same = int((got == exact).all(dim=1).sum())
            hits = (got.unsqueeze(2) == exact.unsqueeze(1)).any(dim=2).float().mean().item() if Q * k * k <= 1 << 31 else float('nan')
            result['search_s']['%d/%d' % (k, R)] = ts[0]
            result['agreement']['%d/%d' % (k, R)] = [same, Q, hits]
            say('k = %4d  Int8Index.search, rerank = %4d           %8.4f s (%.4f .. %.4f);  lists == fp32 lists in %d of %d queries, '
                'recall@%d = %.4f' % (k, R, ts[0], ts[1], ts[2], same, Q, k, hits))
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python
"""The fp4 descriptor index on one MI355X beside the int8 index, on bench_index.py's seeded unit-norm descriptors.
    python scripts/bench_fp4.py [--q 70] [--n 1006322] [--d 2048] [--k 10 100] [--clusters 6] [--out profiles/fp4.txt]
  quantize          dir_quantize_rows_fp4 and dir_quantize_rows_i8 over the whole database, alternating (device events)
  scan              dir_similarity_fp4 and dir_similarity_i8 alone, alternating inside every repeat of one process, both
                    writing the same Q x N fp32 scores
  search            descriptors -> lists, rerank = 0 and rerank = 4k (CUDA source), Fp4Index beside Int8Index and
                    ranking.retrieve_device (synchronised wall clock), with recall@k against the fp32 lists
  bytes             what the two indexes hold on the device
Every point is the median (min .. max) of `--repeats` timings after a warm-up.  --clusters 6: bench_index.py's sets (the
queries a draw of their own); any other count: bench_ivf.py's (the queries are further rows of the database's draw)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import torch
from bench_index import descriptors, device_ms, recall, wall_s
from dirtorch_amd import ops, ranking
from dirtorch_amd.index import Fp4Index, Int8Index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--clusters', type=int, default=6)
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
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    if args.clusters == 6:
        b = descriptors(N, D, 6, centres)
        q = descriptors(Q, D, 5, centres)
    else:
        b = descriptors(N + Q, D, 6, centres, clusters=args.clusters)
        b, q = b[:N], b[N:].clone()
    say('# fp4 descriptor index: Q = %d, N = %d, D = %d, %d cluster centres; medians (min .. max) of %d timings after a warm-up'
        % (Q, N, D, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    result = {'q': Q, 'n': N, 'd': D, 'clusters': args.clusters}

    t4, t8 = device_ms([lambda: ops.quantize_rows_fp4(b), lambda: ops.quantize_rows(b)], args.inner, args.repeats)
    ldc, lde = ops.fp4_widths(D)
    result.update(quantize_fp4_ms=t4[0], quantize_i8_ms=t8[0])
    say('quantize_rows_fp4, %d rows: %8.3f ms (%.3f .. %.3f) = %5.0f GB/s of fp32 read + codes, block bytes written'
        % (N, t4[0], t4[1], t4[2], N * (D * 4 + ldc + lde + 4) / 1e6 / t4[0]))
    say('quantize_rows (int8)            %8.3f ms (%.3f .. %.3f) = %5.0f GB/s' % (t8[0], t8[1], t8[2], N * D * 5 / 1e6 / t8[0]))

    i4, i8 = Fp4Index(D).add(b), Int8Index(D).add(b)
    bytes_i8 = i8.codes.numel() + 4 * i8.scales.numel()
    result.update(bytes_fp4=i4.nbytes(), bytes_i8=bytes_i8)
    say('bytes held: fp4 %d (%d a row: %d codes + %d block bytes + 4), int8 %d (%d a row), fp32 %d'
        % (i4.nbytes(), ldc + lde + 4, ldc, lde, bytes_i8, i8.codes.shape[1] + 4, N * D * 4))

    c4, e4, s4 = ops.quantize_rows_fp4(q)
    c8, s8 = ops.quantize_rows(q)
    out = torch.empty(Q, N, dtype=torch.float32, device='cuda')
    t4, t8 = device_ms([lambda: ops.similarity_fp4(c4, e4, s4, i4.codes, i4.exps, i4.scales, D, out=out),
                        lambda: ops.similarity_i8(c8, s8, i8.codes, i8.scales, D, out=out)], args.inner, args.repeats)
    b4, b8 = N * (ldc + lde + 4) + Q * N * 4, N * (i8.codes.shape[1] + 4) + Q * N * 4
    result.update(similarity_fp4_ms=t4[0], similarity_i8_ms=t8[0])
    say('similarity_fp4                %8.3f ms (%.3f .. %.3f): %.2f GB (codes, block bytes once + scores) = %5.0f GB/s'
        % (t4[0], t4[1], t4[2], b4 / 1e9, b4 / 1e6 / t4[0]))
    say('similarity_i8                 %8.3f ms (%.3f .. %.3f): %.2f GB (codes once + scores) = %5.0f GB/s'
        % (t8[0], t8[1], t8[2], b8 / 1e9, b8 / 1e6 / t8[0]))
    say('fp4 scan / int8 scan = %.3f of the time (bytes: %.3f); every fp4 timing below every int8 timing: %s'
        % (t4[0] / t8[0], b4 / b8, t4[2] < t8[1]))
    result['scan_ratio'] = t4[0] / t8[0]
    del out

    result['search_s'], result['recall'] = {}, {}
    for k in args.k:
        tr = wall_s(lambda: ranking.retrieve_device(q, b, k), args.repeats)
        exact = tr[3][0]
        say('k = %4d  retrieve_device (fp32 rows)              %8.4f s (%.4f .. %.4f)' % (k, tr[0], tr[1], tr[2]))
        result['search_s']['fp32/%d' % k] = tr[0]
        for name, index in (('Int8Index', i8), ('Fp4Index', i4)):
            for R in (0, 4 * k):
                ts = wall_s(lambda: index.search(q, k, rerank=R, source=b if R else None), args.repeats)
                got = ts[3][0]
                same, hits = int((got == exact).all(dim=1).sum()), recall(got, exact)
                result['search_s']['%s/%d/%d' % (name, k, R)] = ts[0]
                result['recall']['%s/%d/%d' % (name, k, R)] = hits
                say('k = %4d  %-9s.search, rerank = %4d           %8.4f s (%.4f .. %.4f);  lists == fp32 lists in %d of %d queries, '
                    'recall@%d = %.4f' % (k, name, R, ts[0], ts[1], ts[2], same, Q, k, hits))
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

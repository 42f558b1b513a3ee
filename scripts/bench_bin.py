#!/usr/bin/env python
"""The binary descriptor index on one MI355X beside the int8, fp4 and product-quantised indexes, on bench_index.py's seeded
unit-norm descriptors.  It can only run on a GPU machine.
    python scripts/bench_bin.py [--q 70] [--n 1006322] [--d 2048] [--k 10 100] [--clusters 6] [--pq-m 64] [--out profiles/bin.txt]
  quantize          dir_quantize_rows_bin beside dir_quantize_rows_i8 and dir_quantize_rows_fp4 over the whole database,
                    alternating (device events)
  bytes             what the indexes hold on the device
  scan              dir_similarity_bin, dir_similarity_i8, dir_similarity_fp4 and (--pq-m M, 0 = leave out) dir_pq_scan
                    alone, alternating inside every repeat of one process, all writing the same Q x N fp32 scores; then
                    the same for --scan-shapes further Q x N cuts of the sets (1 x N and 20000 x 20000 by default)
  search            descriptors -> lists at every k, raw and with rerank = 4k (CUDA source), BinaryIndex beside Int8Index
                    and Fp4Index and ranking.retrieve_device (synchronised wall clock), with recall@k against the fp32
                    lists; BinaryIndex also with the longest shortlist a search takes (ops.topk_max_k() = 2048)
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
from dirtorch_amd.index import BinaryIndex, Fp4Index, Int8Index, PQIndex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, default=70)
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--clusters', type=int, default=6)
    ap.add_argument('--pq-m', type=int, default=64)
    ap.add_argument('--scan-shapes', type=str, nargs='*', default=['1x0', '20000x20000'], help='QxN, 0 = all rows')
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
    say('# binary descriptor index: Q = %d, N = %d, D = %d, %d cluster centres; medians (min .. max) of %d timings after a warm-up'
        % (Q, N, D, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    result = {'q': Q, 'n': N, 'd': D, 'clusters': args.clusters}
    fp4 = D <= ops.index_fp4_max_dim()

    fns = [lambda: ops.quantize_rows_bin(b), lambda: ops.quantize_rows(b)] + ([lambda: ops.quantize_rows_fp4(b)] if fp4 else [])
    ts = device_ms(fns, args.inner, args.repeats)
    ldb = ops.bin_width(D)
    for name, t, out_bytes in zip(('quantize_rows_bin', 'quantize_rows (int8)', 'quantize_rows_fp4'), ts,
                                  (ldb + 4, (D + 63) // 64 * 64 + 4, sum(ops.fp4_widths(D)) + 4)):
        result[name.split(' ')[0] + '_ms'] = t[0]
        say('%-22s %d rows: %8.3f ms (%.3f .. %.3f) = %5.0f GB/s of fp32 read + %d bytes a row written'
            % (name, N, t[0], t[1], t[2], N * (D * 4 + out_bytes) / 1e6 / t[0], out_bytes))

    ib, i8 = BinaryIndex(D).add(b), Int8Index(D).add(b)
    i4 = Fp4Index(D).add(b) if fp4 else None
    bytes_i8 = i8.codes.numel() + 4 * i8.scales.numel()
    result.update(bytes_bin=ib.nbytes(), bytes_i8=bytes_i8, bytes_fp4=i4.nbytes() if fp4 else None)
    say('bytes held: bin %d (%d a row: %d bits + 4), fp4 %s, int8 %d (%d a row), fp32 %d'
        % (ib.nbytes(), ldb + 4, ldb, '%d (%d a row)' % (i4.nbytes(), sum(ops.fp4_widths(D)) + 4) if fp4 else '-', bytes_i8,
           i8.codes.shape[1] + 4, N * D * 4))
    ipq = None
    if args.pq_m:
        ipq = PQIndex(D, args.pq_m)
        ipq.train(b)
        ipq.add(b)

    c8, s8 = ops.quantize_rows(q)
    c4 = ops.quantize_rows_fp4(q) if fp4 else None
    shapes = [(Q, N)]
    for s in args.scan_shapes:
        sq, sn = (int(v) for v in s.split('x'))
        shapes.append((sq, sn or N))
    result['scan_ms'] = {}
    for sq, sn in shapes:
        sn = min(sn, N)
        # more queries than the query set has: database rows stand in (a scan's time does not depend on the values)
        qq = q if sq <= Q else b[:sq]
        qc8, qs8 = (c8, s8) if sq <= Q else ops.quantize_rows(qq)
        qc4 = c4 if sq <= Q else (ops.quantize_rows_fp4(qq) if fp4 else None)
        out = torch.empty(sq, sn, dtype=torch.float32, device='cuda')
        names = ['similarity_bin', 'similarity_i8']
        fns = [lambda: ops.similarity_bin(qc8[:sq], qs8[:sq], ib.codes[:sn], ib.scales[:sn], D, out=out),
               lambda: ops.similarity_i8(qc8[:sq], qs8[:sq], i8.codes[:sn], i8.scales[:sn], D, out=out)]
        moved = [sn * (ldb + 4), sn * (i8.codes.shape[1] + 4)]
        if fp4:
            names.append('similarity_fp4')
            fns.append(lambda: ops.similarity_fp4(qc4[0][:sq], qc4[1][:sq], qc4[2][:sq], i4.codes[:sn], i4.exps[:sn],
                                                  i4.scales[:sn], D, out=out))
            moved.append(sn * (sum(ops.fp4_widths(D)) + 4))
        if ipq is not None:
            lut = ops.pq_lut(qq[:sq], ipq.codebooks)
            names.append('pq_scan (M = %d)' % args.pq_m)
            fns.append(lambda: ops.pq_scan(lut, ipq.codes[:sn], out=out))
            moved.append(sn * ipq.codes.shape[1])
        ts = device_ms(fns, args.inner, args.repeats)
        say('scan of %d queries x %d rows (scores written: %.3f GB)' % (sq, sn, sq * sn * 4 / 1e9))
        qblocks = (sq + 95) // 96
        for name, t, mb in zip(names, ts, moved):
            total = mb * qblocks + sq * sn * 4
            result['scan_ms']['%s/%dx%d' % (name, sq, sn)] = t[0]
            say('   %-20s %8.3f ms (%.3f .. %.3f): %.3f GB (rows once per query block + scores) = %5.0f GB/s;  / similarity_bin = %.2f'
                % (name, t[0], t[1], t[2], total / 1e9, total / 1e6 / t[0], t[0] / ts[0][0]))
        del out

    longest = min(N, ops.topk_max_k())               # the longest shortlist a search takes
    result['search_s'], result['recall'] = {}, {}
    for k in args.k:
        tr = wall_s(lambda: ranking.retrieve_device(q, b, k), args.repeats)
        exact = tr[3][0]
        say('k = %4d  retrieve_device (fp32 rows)                %8.4f s (%.4f .. %.4f)' % (k, tr[0], tr[1], tr[2]))
        result['search_s']['fp32/%d' % k] = tr[0]
        for name, index in (('Int8Index', i8), ('Fp4Index', i4), ('BinaryIndex', ib)):
            if index is None:
                continue
            for R in (0, 4 * k) + ((longest,) if name == 'BinaryIndex' and longest > 4 * k else ()):
                ts = wall_s(lambda: index.search(q, k, rerank=R, source=b if R else None), args.repeats)
                got = ts[3][0]
                same, hits = int((got == exact).all(dim=1).sum()), recall(got, exact)
                result['search_s']['%s/%d/%d' % (name, k, R)] = ts[0]
                result['recall']['%s/%d/%d' % (name, k, R)] = hits
                say('k = %4d  %-11s.search, rerank = %4d           %8.4f s (%.4f .. %.4f);  lists == fp32 lists in %d of %d queries, '
                    'recall@%d = %.4f' % (k, name, R, ts[0], ts[1], ts[2], same, Q, k, hits))
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

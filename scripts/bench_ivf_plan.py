#!/usr/bin/env python
"""search(plan='device') beside search(plan='host') on one MI355X: the inverted files with their probe tables from one kernel
(dir_ivf_plan) and with the integer torch operations and the read-back they replace, on bench_index.py's seeded descriptors.
    python scripts/bench_ivf_plan.py [--q 1 70] [--n 1006322] [--d 2048] [--nlist 1024] [--nprobe 1 8 32] [--out profiles/ivf_plan.txt]
  search    descriptors (on the device) -> lists: IVFInt8Index / IVFFp4Index .search with plan='host' and plan='device',
            alternating in one process (synchronised wall clock), at k = 10 and at k = 100 with rerank 400 (CUDA source);
            the lists of the two plans are compared on bits at every point
  planner   ops.ivf_plan alone beside index._slots + ops.ivf_probe_tables (wall clock: the host path ends in a read-back; and
            device events for the planner, which needs none)
  grid      dir_ivf_scan_i8 / dir_ivf_scan_fp4 on the planned tables with the host's bound of the grid beside the exact
            grid (device events): the bound, the true count and what the surplus workgroups cost
Every point is the median (min .. max) of `--repeats` timings after a warm-up; the yardstick is the host plan in the same
process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import numpy as np
import torch
from bench_index import alternating, descriptors, event_ms, wall_ms
from dirtorch_amd import ops
from dirtorch_amd.index import IVFFp4Index, IVFInt8Index


def same_lists(a, b):
    return torch.equal(a[0], b[0]) and bool(((a[1].view(torch.int32) == b[1].view(torch.int32)) |
                                             (torch.isnan(a[1]) & torch.isnan(b[1]))).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--q', type=int, nargs='+', default=[1, 70])
    ap.add_argument('--n', type=int, default=1006322)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--nlist', type=int, default=1024)
    ap.add_argument('--nprobe', type=int, nargs='+', default=[1, 8, 32])
    ap.add_argument('--clusters', type=int, default=16384)
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
    N, D, nlist = args.n, args.d, args.nlist
    centres = torch.randn(args.clusters, D, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
    b = descriptors(N + max(args.q), D, 6, centres, clusters=args.clusters)
    b, qall = b[:N], b[N:].clone()
    say('# device planner of the inverted files: N = %d, D = %d, nlist = %d, %d cluster centres; medians (min .. max) of %d '
        'timings after a warm-up, plan=host and plan=device alternating' % (N, D, nlist, args.clusters, args.repeats))
    say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
    i8 = IVFInt8Index(D, nlist).train(b, iters=args.iters).add(b)
    fp4 = IVFFp4Index(D, nlist)
    fp4._set_centroids(i8.centroids.clone())
    fp4.add(b)
    lens = i8._lens
    say('list sizes %d .. %d' % (lens.min(), lens.max()))
    result = {'n': N, 'd': D, 'nlist': nlist, 'search': [], 'planner': [], 'grid': []}

    say('## search: descriptors -> lists, wall clock')
    for name, index in (('IVFInt8Index', i8), ('IVFFp4Index', fp4)):
        for Q in args.q:
            q = qall[:Q]
            for nprobe in args.nprobe:
                for k, R in ((10, 0), (100, 400)):
                    kw = dict(nprobe=nprobe, rerank=R, source=b if R else None)
                    th, td = alternating([lambda: index.search(q, k, plan='host', **kw), lambda: index.search(q, k, plan='device', **kw)],
                                         args.repeats, wall_ms)
                    ok = same_lists(th[3], td[3])
                    say('%-12s Q = %2d nprobe = %2d k = %3d rerank = %3d  host %7.3f ms (%.3f .. %.3f) | device %7.3f ms (%.3f .. %.3f)'
                        ' | device / host %.3f | lists %s' % (name, Q, nprobe, k, R, th[0], th[1], th[2], td[0], td[1], td[2],
                                                             td[0] / th[0], 'identical' if ok else 'DIFFER'))
                    result['search'].append({'index': name, 'q': Q, 'nprobe': nprobe, 'k': k, 'rerank': R, 'host_ms': th[0],
                                             'device_ms': td[0], 'identical': ok})

    say('## planner alone: ops.ivf_plan beside _slots + ops.ivf_probe_tables')
    say('## grid: the scan on planned tables, the host bound of the grid beside the exact grid (device events)')
    for Q in args.q:
        q = qall[:Q]
        qc, qs = ops.quantize_rows(q)
        f4 = ops.quantize_rows_fp4(q)
        for nprobe in args.nprobe:
            probe = i8.probe(qc, qs, nprobe)
            bound = i8._plan_items(Q, nprobe)
            width = int(np.sort(lens)[-nprobe:].sum())            # the width a search takes: the nprobe longest lists
            th, td = alternating([lambda: ops.ivf_probe_tables(i8.list_off, probe, i8._slots(probe)),
                                  lambda: ops.ivf_plan(i8.list_off, probe, bound)], args.repeats, wall_ms)
            te = alternating([lambda: ops.ivf_plan(i8.list_off, probe, bound)], args.repeats, lambda fn: event_ms(fn, args.inner))[0]
            col_off, tables, counts = td[3]
            items, reach = counts.tolist()
            assert items == th[3][4] and reach == th[3][5] and items <= bound and reach <= width
            say('Q = %2d nprobe = %2d  planner: host tables %7.3f ms (%.3f .. %.3f) | ivf_plan %7.3f ms (%.3f .. %.3f) wall, %.4f ms '
                '(%.4f .. %.4f) on the device' % (Q, nprobe, th[0], th[1], th[2], td[0], td[1], td[2], te[0], te[1], te[2]))
            result['planner'].append({'q': Q, 'nprobe': nprobe, 'host_ms': th[0], 'device_wall_ms': td[0], 'device_event_ms': te[0]})
            exact = tables[:4] + (items, None)
            out = (torch.empty(Q, width, dtype=torch.float32, device='cuda'), torch.empty(Q, width, dtype=torch.int32, device='cuda'))
            for name, scan in (('ivf_scan', lambda t: ops.ivf_scan(qc, qs, i8.codes, i8.scales, i8.ids, i8.list_off, probe, col_off, D,
                                                                   width=width, out=out, tables=t)),
                               ('ivf_scan_fp4', lambda t: ops.ivf_scan_fp4(*f4, fp4.codes, fp4.exps, fp4.scales, fp4.ids, fp4.list_off,
                                                                           probe, col_off, D, width=width, out=out, tables=t))):
                tx, tb = alternating([lambda: scan(exact), lambda: scan(tables)], args.repeats, lambda fn: event_ms(fn, args.inner))
                say('                     %-12s exact grid %6d: %8.4f ms (%.4f .. %.4f) | bound %6d: %8.4f ms (%.4f .. %.4f) | '
                    '%+.4f ms for %d surplus workgroups' % (name, items, tx[0], tx[1], tx[2], bound, tb[0], tb[1], tb[2],
                                                            tb[0] - tx[0], bound - items))
                result['grid'].append({'scan': name, 'q': Q, 'nprobe': nprobe, 'items': items, 'bound': bound, 'exact_ms': tx[0],
                                       'bound_ms': tb[0]})
            del out
    print(json.dumps(result))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n\n')


if __name__ == '__main__':
    main()

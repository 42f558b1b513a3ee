#!/usr/bin/env python
"""Class-labelled evaluation, host route against device route, on one MI355X: eval_model's tail from the descriptors
(host ndarrays) to the result dict on the same seeded data.
    python scripts/bench_label_rank.py [--n 20000] [--d 2048] [--classes 200] [--out profiles/label_rank.txt]
  host route    test_dir.eval_model's host loop: common.matmul (upload, similarity, download of the Q x N matrix), then
                per query get_query_groundtruth + sklearn average_precision_score and an argsort for the top-k hits
  device route  ranking.eval_labelled_device: upload, then similarity + dir_label_rank per chunk of query rows
Every repeat ends in the host values it returns (a synchronised wall clock); the per-kernel split of the device route
comes from device events around each ops.similarity / ops.label_rank call in one more repeat of its own, in which every
chunk's dir_label_rank is followed by the same call on ONE query row - the table check plus a one-workgroup ranking
launch, i.e. the check's share of the call; the peak
device memory is torch's allocator peak over a repeat.  Agreement is reported per query: the device route in ONE chunk ranks
the very scores the host route downloads; in chunks, a query's scores are dir_similarity's for its block of rows, whose
fp32 sums start at a tile-dependent K slab (csrc/gemm_f32.hip), so last-bit differences can swap near-equal neighbours."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
import numpy as np
import torch
from dirtorch_amd import datasets, ops, ranking
from dirtorch_amd.test_dir import _mean_ap
from dirtorch_amd.utils.common import matmul


def make_dataset(n, classes, d, seed, tmp):
    """ImageListLabels over n images in `classes` classes of mixed size (a few large, many small), with unit-norm
    descriptors that lean towards their class centre."""
    r = np.random.RandomState(seed)
    w = 1.0 / np.arange(1, classes + 1) ** 0.8
    labels = r.choice(classes, n, p=w / w.sum())
    labels[:classes] = np.arange(classes)                       # no empty class
    lst = os.path.join(tmp, 'list.txt')
    with open(lst, 'w') as f:
        f.write(''.join('img%d.jpg c%d\n' % (i, c) for i, c in enumerate(labels)))
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(classes, d, generator=g)
    x = torch.randn(n, d, generator=g) + 0.15 * centres[torch.from_numpy(labels)]
    x = torch.nn.functional.normalize(x, dim=1).numpy()
    return datasets.ImageListLabels(lst, root=tmp), x, np.bincount(labels, minlength=classes)


def result_dict(aps, tops):
    res = {}
    _mean_ap(aps, True, res)
    res['tops'] = tops
    for k in tops[0]:
        res['top%d' % k] = float(np.mean([t[k] for t in tops]))
    return res


def compare(a, b):
    d = np.abs(np.array(a['APs']) - np.array(b['APs']))
    return 'max |AP difference| %.3g over %d queries (%d differ), |mAP difference| %.3g, %d queries with another top-k dict' % (
        d.max(), len(d), int((d > 0).sum()), abs(a['mAP'] - b['mAP']), sum(x != y for x, y in zip(a['tops'], b['tops'])))


def host_route(db, descs, progress=None):
    scores = matmul(descs, descs)
    aps, tops = [], []
    for q, s in enumerate(scores):
        aps.append(db.eval_query_AP(q, s))
        if progress and q % 2500 == 0:
            progress('  host AP %d / %d' % (q, len(scores)))
    for q, s in enumerate(scores):
        tops.append(db.eval_query_top(q, s))
        if progress and q % 2500 == 0:
            progress('  host top-k %d / %d' % (q, len(scores)))
    return result_dict(aps, tops)


def device_route(db, descs, tables, **kw):
    return result_dict(*ranking.eval_labelled_device(db, descs, descs, tables=tables, **kw))


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, torch.cuda.max_memory_allocated(), out


def kernel_split(db, descs, tables):
    """Device time of the two per-chunk calls of one device-route repeat, from events on the stream, and of the table
    check alone (a one-query dir_label_rank after every chunk's)."""
    spans = {'similarity': [], 'label_rank': [], 'table_check': []}
    orig = {'similarity': ops.similarity, 'label_rank': ops.label_rank}

    def span(name, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        spans[name].append((e0, e1))
        return out

    def wrap(name):
        def f(*a, **kw):
            out = span(name, lambda: orig[name](*a, **kw))
            if name == 'label_rank':
                scores, labels, off, members, qclass, qself = a
                span('table_check', lambda: orig[name](scores[:1], labels, off, members, qclass[:1], qself[:1]))
            return out
        return f
    ops.similarity, ops.label_rank = wrap('similarity'), wrap('label_rank')
    try:
        device_route(db, descs, tables)
        torch.cuda.synchronize()
    finally:
        ops.similarity, ops.label_rank = orig['similarity'], orig['label_rank']
    return {name: (len(v), sum(a.elapsed_time(b) for a, b in v)) for name, v in spans.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=20000)
    ap.add_argument('--d', type=int, default=2048)
    ap.add_argument('--classes', type=int, default=200)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--device-repeats', type=int, default=9)
    ap.add_argument('--out', type=str, default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    with tempfile.TemporaryDirectory() as tmp:
        db, x, sizes = make_dataset(args.n, args.classes, args.d, 5, tmp)
        say('# class-labelled evaluation, descriptors -> result dict: Q = N = %d, D = %d, %d classes of %d ... %d images '
            '(median %d), self-query set' % (args.n, args.d, args.classes, sizes.min(), sizes.max(), int(np.median(sizes))))
        say('# %s, torch %s' % (torch.cuda.get_device_name(0), torch.__version__))
        t0 = time.perf_counter()
        tables = ranking.build_label_tables(db)
        say('build_label_tables (host, once per dataset): %.3f s' % (time.perf_counter() - t0))
        device_route(db, x, tables)                             # warm-up: code objects, allocator
        dev = [timed(lambda: device_route(db, x, tables)) for _ in range(args.device_repeats)]
        dts = sorted(t for t, _, _ in dev)
        say('device route, %d repeats after a warm-up: median %.3f s, min %.3f s, max %.3f s; peak device memory %.0f MiB'
            % (len(dts), statistics.median(dts), dts[0], dts[-1], max(m for _, m, _ in dev) / 2 ** 20))
        split = kernel_split(db, x, tables)
        say('  device time inside one repeat: %d x similarity %.1f ms, %d x dir_label_rank %.1f ms, of which the table check '
            '(label_check_kernel + read-back, timed as %d one-query calls) %.1f ms and label_rank_kernel the rest'
            % (split['similarity'][0], split['similarity'][1], split['label_rank'][0], split['label_rank'][1],
               split['table_check'][0], split['table_check'][1]))
        host = []
        for i in range(args.host_repeats):
            host.append(timed(lambda: host_route(db, x, progress=print if i == 0 else None)))
            say('host route, repeat %d: %.1f s' % (i, host[-1][0]))
        hts = sorted(t for t, _, _ in host)
        say('host route, %d repeats (the first doubles as warm-up and is counted): median %.1f s, min %.1f s, max %.1f s; '
            'peak device memory %.0f MiB' % (len(hts), statistics.median(hts), hts[0], hts[-1],
                                            max(m for _, m, _ in host) / 2 ** 20))
        rd, rh = dev[0][2], host[0][2]
        assert list(rd) == list(rh), (list(rd), list(rh))
        one = device_route(db, x, tables, scratch_bytes=4 * args.n * args.n)
        say('device route in ONE chunk (the scores the host downloads) vs host route: ' + compare(one, rh))
        say('device route in 256 MiB chunks vs host route: ' + compare(rd, rh))
        say('mAP %.12f (device) / %.12f (host); %s' % (rd['mAP'], rh['mAP'], ', '.join(
            '%s %g / %g' % (k, rd[k], rh[k]) for k in rd if k.startswith('top') and k != 'tops')))
        say('speed-up of the device route (medians): %.0fx' % (statistics.median(hts) / statistics.median(dts)))
        print(json.dumps({'n': args.n, 'd': args.d, 'device_s': dts, 'host_s': hts, 'device_mAP': rd['mAP'],
                          'host_mAP': rh['mAP']}))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

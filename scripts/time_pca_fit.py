#!/usr/bin/env python
"""What a PCA fit costs: whitening.fit_pca on N x 2048 unit-norm descriptors already on the device (dir_cov_accumulate + the
host's D x D eigh) beside the route it replaces - the descriptors on the host, numpy fp64 X.T @ X + eigh on this box's CPUs.

    python scripts/time_pca_fit.py [--rows 100000 1000000] [--dim 2048] [--out profiles/pca_fit_time.txt] [--no-cpu]

Per N: the device Gram launch alone (median of 3 after a warm-up, HIP events; the triangle is N D (D + 1) FLOP), the whole
fit_pca call (wall clock, eigh included), and the CPU route in row blocks of 65536 (wall clock; its eigh is the same call).
The library in use reports its chain length R; an experiment build (-DDIR_COV_CHAIN_ROWS=n, selected with DIRTORCH_AMD_LIB)
shows what another R costs."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'deep-image-retrieval_amd'))
import numpy as np
import torch
from dirtorch_amd import ops, whitening


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[100000, 1000000])
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--out', type=str, default='')
    ap.add_argument('--no-cpu', action='store_true')
    ap.add_argument('--no-eigh', action='store_true', help='time the device launches only')
    args = ap.parse_args()
    D, R = args.dim, ops.cov_chain_rows()
    lines, recs = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('# PCA fit, D = %d, chain rows R = %d, %d CPU threads (%s)' % (D, R, torch.get_num_threads(), torch.cuda.get_device_name(0)))
    for N in args.rows:
        g = torch.Generator(device='cuda').manual_seed(1)
        X = torch.randn(N, D, device='cuda', generator=g).abs_()
        X += 0.25 * torch.randn(N, D, device='cuda', generator=g)
        X = torch.nn.functional.normalize(X, dim=1).contiguous()
        shift = X[:4096].double().mean(dim=0).float().contiguous()
        gram = torch.zeros(D, D, dtype=torch.float64, device='cuda')
        sums = torch.zeros(D, dtype=torch.float64, device='cuda')
        ops.cov_accumulate(X, shift, gram, sums)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(3):
            e0.record()
            ops.cov_accumulate(X, shift, gram, sums)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        fl = float(N) * D * (D + 1)
        rec = {'N': N, 'D': D, 'R': R, 'gram_ms': ms[1], 'gram_tflops_triangle': fl / ms[1] / 1e9}
        say('N = %8d: device Gram launch %9.2f ms = %6.1f TFLOP/s on the triangle (X is %.2f GB)' % (N, ms[1], fl / ms[1] / 1e9, N * D * 4 / 1e9))
        if not args.no_eigh:
            t = time.time()
            pca = whitening.fit_pca(X)
            rec['fit_pca_s'] = time.time() - t
            say('              fit_pca, descriptors on the device   %8.2f s (the host eigh of %d x %d included)' % (rec['fit_pca_s'], D, D))
        if not args.no_cpu:
            t = time.time()
            Xh = X.cpu().numpy()
            rec['download_s'] = time.time() - t
            t = time.time()
            G = np.zeros((D, D), np.float64)
            s = np.zeros(D, np.float64)
            for r in range(0, N, 65536):
                blk = Xh[r:r + 65536].astype(np.float64)
                G += blk.T @ blk
                s += blk.sum(axis=0)
            rec['cpu_gram_s'] = time.time() - t
            t = time.time()
            C = (G - np.outer(s, s) / N) / (N - 1)
            w, _ = np.linalg.eigh(C)
            rec['cpu_eigh_s'] = time.time() - t
            say('              host route: download %.2f s + numpy fp64 X.T @ X %8.2f s + eigh %.2f s' % (rec['download_s'], rec['cpu_gram_s'], rec['cpu_eigh_s']))
            if not args.no_eigh:
                lam = np.maximum(w[::-1], 0)
                rec['eigenvalue_max_rel_diff_top64'] = float(np.abs(pca.explained_variance_[:64] - lam[:64]).max() / lam[0])
                say('              largest 64 eigenvalues agree to %.2e of lambda_max' % rec['eigenvalue_max_rel_diff_top64'])
            del Xh
        recs.append(rec)
        del X, gram
        torch.cuda.empty_cache()
    lines.append(json.dumps(recs))
    if args.out:
        folder = os.path.dirname(args.out)
        if folder:
            os.makedirs(folder, exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()

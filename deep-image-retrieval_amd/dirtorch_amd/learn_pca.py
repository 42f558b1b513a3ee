"""Learn a PCA whitening on a dataset's descriptors and store it in a checkpoint.

    python -m dirtorch_amd.learn_pca --dataset Landmarks18_pca --checkpoint IN.pt --output OUT.pt [--name KEY] --gpu 0
    python -m dirtorch_amd.test_dir  --dataset ROxford5K --checkpoint OUT.pt --whiten KEY

The reference ships the image list to fit on (Landmarks18_pca) and reads the result (ck['pca'][KEY], dirtorch/test_dir.py:
189-190, 237-243) but has no code for the fit.  Descriptors are extracted chunk by chunk through the evaluation's own path
(test_dir.extract_per_scale -> extract_image_features, pooled over the transform chains and L2-normalised exactly as
test_dir.eval_model does before it whitens) and fed to whitening.PCAFitter: the descriptors never leave the device and no
N x D matrix is ever held.  OUT is a copy of IN with ck['pca'][KEY] set; every other key, other PCAs included, is kept.
Single process only.
"""
import os
import sys

from . import datasets
from . import test_dir as test
from . import whitening
from .utils import common
from .utils.common import pool

CHUNK_IMAGES = 4096      # images whose descriptors are held at a time


class _Rows(datasets.Dataset):
    """Images [start, stop) of a dataset, as the loader sees them."""

    def __init__(self, db, start, stop):
        self.db, self.start = db, start
        self.nimg = stop - start
        self.root, self.img_dir = db.root, db.img_dir

    def get_key(self, i):
        return self.db.get_key(self.start + i)

    def get_filename(self, i, root=None):
        return self.db.get_filename(self.start + i, root=root)

    def get_image(self, i, resize=None):
        return self.db.get_image(self.start + i, resize=resize)


def learn_pca(db, net, trfs, pooling='mean', gemp=3, threads=8, batch_size=16, max_images=None, chunk_images=CHUNK_IMAGES):
    """PCAFitter over the descriptors of `db` (its first `max_images` images), as eval_model computes them."""
    n = len(db) if not max_images else min(len(db), int(max_images))
    fitter = None
    for start in range(0, n, chunk_images):
        rows = _Rows(db, start, min(n, start + chunk_images))
        per_scale = test.extract_per_scale(rows, trfs, net, desc='PCA %d/%d' % (start, n), threads=threads,
                                           batch_size=batch_size)
        descs = common.l2_normalize(pool(per_scale, pooling, gemp))
        if fitter is None:
            fitter = whitening.PCAFitter(descs.shape[1])
        fitter.partial_fit(descs)
    if fitter is None:
        raise ValueError('learn_pca: the dataset is empty')
    return fitter


def main(argv=None):
    import argparse
    import torch
    p = argparse.ArgumentParser(description='Learn a PCA whitening and store it in a checkpoint')
    p.add_argument('--dataset', '-d', type=str, required=True, help='Command to load dataset')
    p.add_argument('--checkpoint', type=str, required=True, help='path to weights')
    p.add_argument('--output', type=str, required=True, help='path of the checkpoint to write')
    p.add_argument('--name', type=str, default=None, help="key under ck['pca'] (default: the dataset command)")
    p.add_argument('--trfs', type=str, required=False, default='', nargs='+', help='test transforms (can be several)')
    p.add_argument('--pooling', type=str, default='gem', help='pooling scheme if several trf chains')
    p.add_argument('--gemp', type=int, default=3, help='GeM pooling power')
    p.add_argument('--gpu', type=int, default=0, nargs='+', help='GPU ids')
    p.add_argument('--threads', type=int, default=8, help='number of thread workers')
    p.add_argument('--max-images', type=int, default=None, help='fit on the first N images only')
    args = p.parse_args(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise RuntimeError('learn_pca runs as a single process')
    iscuda = common.torch_set_gpu(args.gpu)
    db = datasets.create(args.dataset)
    print('PCA dataset:', db)
    net = test.load_model(args.checkpoint, iscuda)
    fitter = learn_pca(db, net, args.trfs, pooling=args.pooling, gemp=args.gemp, threads=args.threads,
                       max_images=args.max_images)
    pca = fitter.finalize()
    key = args.name or args.dataset
    ck = common.torch_load_trusted(args.checkpoint)      # as stored: parameter names keep their 'module.' prefix
    ck['pca'] = dict(ck.get('pca') or {})
    ck['pca'][key] = pca
    folder = os.path.dirname(args.output)
    if folder:
        os.makedirs(folder, exist_ok=True)
    torch.save(ck, args.output)
    print("PCA of %d descriptors x %d stored as ck['pca'][%r] in %s" % (fitter.n, fitter.D, key, args.output))
    return pca


if __name__ == '__main__':
    main(sys.argv[1:])

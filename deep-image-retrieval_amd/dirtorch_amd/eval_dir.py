"""Retrieval evaluation with the device route for class-labelled datasets.

    python -m dirtorch_amd.eval_dir --dataset 'ImageListLabels("val.txt")' --checkpoint X.pt --whiten Landmarks_clean

eval_model / main here take the arguments and flags of dirtorch_amd.test_dir and return the same dict.  The one
difference: a class-labelled dataset (ImageListLabels / ImageListLabelsQ: db.c_relevant_idx and db.labels) under
DIRTORCH_AMD_DEVICE_RANK=1, or `auto` (default) from 50 000 images - the switch and threshold test_dir.eval_model
applies to the revisited Oxford / Paris datasets - is scored and ranked on the GPU in row chunks
(ranking.eval_labelled_device) instead of downloading the Q x N score matrix, calling sklearn once per query and
sorting every row (test_dir.py:153-178).  Every other case IS test_dir.eval_model.
--expand lists (that device route only; default --expand matrix): --aqe / --adba take their neighbours from exact top-k lists
and a gather (ranking.expand_device) instead of the n x m score matrix of test_dir.expand_descriptors.
--diffusion K KQ (default off; a dataset with a query set of its own): the scores are ranking.diffuse_device's - diffusion
on the mutual K-NN graph of the database from the KQ best rows of every query, "+DFS" of the revisited Oxford / Paris
tables - with --diffusion-alpha 0.99, --diffusion-gamma 3, --diffusion-iters 20.  It composes after --adba / --aqe: it
scores the descriptors those produce.  The APs come from ranking.eval_aps_device for the revisitop / classic datasets and
from db.eval_query_AP on downloaded rows otherwise.
--diffusion-trunc T (with --diffusion; default off): the scores are the dense form of ranking.diffuse_truncated_device -
every query solved on the subgraph of its T best database rows, those rows ranked by their diffusion score above all
others, the others in cosine order.  With it a dataset whose queries are its database rows is accepted (the row itself
is the one-hot seed).
"""
import json
import os
import sys

import numpy as np

from . import datasets, ranking, test_dir
from . import distributed as ddist
from .utils import common
from .utils.common import pool, tonumpy
from .utils.convenient import mkdir


def labelled_on_device(db):
    """Does eval_model rank `db` with ranking.eval_labelled_device?"""
    flag = os.environ.get('DIRTORCH_AMD_DEVICE_RANK', 'auto')
    wanted = flag == '1' or (flag == 'auto' and len(db) >= 50000)
    return bool(wanted and not hasattr(db, 'junk') and getattr(db, 'c_relevant_idx', None) is not None
                and getattr(db, 'labels', None))


EXPAND_ROUTES = ('matrix', 'lists')
EXPAND_FLAG = (('--expand',), dict(type=str, default='matrix', choices=list(EXPAND_ROUTES),
                                   help='--aqe / --adba from the score matrix (default) or from neighbour lists'))


DIFFUSION_FLAGS = [
    (('--diffusion',), dict(type=int, nargs=2, default=None, metavar=('K', 'KQ'),
                            help='diffusion re-ranking: neighbours per database row, seeds per query')),
    (('--diffusion-alpha',), dict(type=float, default=0.99, help='with --diffusion: the damping of the walk, in [0, 1)')),
    (('--diffusion-gamma',), dict(type=float, default=3, help='with --diffusion: the power applied to a similarity')),
    (('--diffusion-iters',), dict(type=int, default=20, help='with --diffusion: conjugate-gradient iterations')),
    (('--diffusion-trunc',), dict(type=int, default=0, metavar='T',
                                  help='with --diffusion: solve every query on the subgraph of its T best rows (0 = all rows)')),
]


def diffusion_options(args):
    """the diffuse_device keywords of parsed DIFFUSION_FLAGS, None without --diffusion; with --diffusion-trunc T also
    trunc=T, which selects ranking.diffuse_truncated_device"""
    if args.diffusion is None:
        if getattr(args, 'diffusion_trunc', 0):
            raise SystemExit('--diffusion-trunc needs --diffusion K KQ')
        return None
    out = dict(k=args.diffusion[0], kq=args.diffusion[1], alpha=args.diffusion_alpha, gamma=args.diffusion_gamma,
               iters=args.diffusion_iters)
    if getattr(args, 'diffusion_trunc', 0):
        if args.diffusion_trunc < 0:
            raise SystemExit('--diffusion-trunc must be positive')
        out['trunc'] = args.diffusion_trunc
    return out


def descriptors(db, net, trfs, pooling='mean', gemp=3, whiten=None, aqe=None, adba=None, threads=8, batch_size=16,
                save_feats=None, load_feats=None, expand='matrix', expand_index=None):
    """(qdescs, bdescs) as test_dir.eval_model prepares them before it scores (test_dir.py:104-143): extracted or
    loaded, pooled over the scales, L2-normalised, saved, whitened, expanded.
    expand='matrix': adba / aqe through test_dir.expand_descriptors (the n x m score matrix; ndarrays come back).
    expand='lists': through ranking.expand_device - neighbour lists, then a gather; the expanded sets come back as CUDA
    tensors (no round trip of a large database through the host).  expand_index (lists only): None for exact lists, or a
    callable bdescs -> (index, search_kw) that returns an index of dirtorch_amd.index holding exactly those rows and the
    keywords of its search (nprobe, rerank); it is called with the un-augmented database for adba (self-set) and with
    the database as it is scored for aqe."""
    if expand not in EXPAND_ROUTES:
        raise ValueError('expand: one of %s expected, got %r' % (', '.join(EXPAND_ROUTES), expand))
    if expand_index is not None and expand != 'lists':
        raise ValueError("expand_index needs expand='lists'")
    query_db = db.get_query_db()
    same_set = query_db is db
    if load_feats:
        bdescs = np.load(os.path.join(load_feats, 'feats.bdescs.npy'))
        qdescs = bdescs if same_set else np.load(os.path.join(load_feats, 'feats.qdescs.npy'))
    else:
        kw = dict(threads=threads, batch_size=batch_size)
        per_scale_b = test_dir.extract_per_scale(db, trfs, net, desc="DB", sharded=True, **kw)
        per_scale_q = per_scale_b if same_set else test_dir.extract_per_scale(query_db, trfs, net, desc="query", **kw)
        bdescs = common.l2_normalize(pool(per_scale_b, pooling, gemp))
        qdescs = common.l2_normalize(pool(per_scale_q, pooling, gemp))
    if save_feats:
        mkdir(save_feats)
        np.save(os.path.join(save_feats, 'feats.bdescs.npy'), tonumpy(bdescs))
        if not same_set:
            np.save(os.path.join(save_feats, 'feats.qdescs.npy'), tonumpy(qdescs))
    if whiten is not None:
        bdescs = common.whiten_features(tonumpy(bdescs), net.pca, **whiten)
        qdescs = common.whiten_features(tonumpy(qdescs), net.pca, **whiten)
    if expand == 'lists':
        def lists_kw(rows):
            if expand_index is None:
                return {}
            index, search_kw = expand_index(rows)
            return dict(search_kw, index=index)
        if adba is not None:
            bdescs = ranking.expand_device(bdescs, **adba, **lists_kw(bdescs))
        if aqe is not None:
            qdescs = ranking.expand_device(qdescs, db=bdescs, **aqe, **lists_kw(bdescs))
        return qdescs, bdescs
    if adba is not None:
        bdescs = test_dir.expand_descriptors(bdescs, **adba)
    if aqe is not None:
        qdescs = test_dir.expand_descriptors(qdescs, db=bdescs, **aqe)
    return qdescs, bdescs


def eval_model(db, net, trfs, pooling='mean', gemp=3, detailed=False, whiten=None, aqe=None, adba=None, threads=8,
               batch_size=16, save_feats=None, load_feats=None, dbg=(), expand='matrix', diffusion=None):
    """test_dir.eval_model, except that a class-labelled dataset under the device-rank switch (labelled_on_device) is
    ranked on the GPU; `mAP`, `APs`, `top<k>` and `tops` are filled as the host branch fills them.  expand='lists'
    (descriptors above) exists on that device route only: test_dir.eval_model has one expansion, the matrix, and asking
    it for lists raises instead of quietly running the matrix.
    diffusion: None, or the keywords of ranking.diffuse_device (k, kq, gamma, alpha, iters) - the queries are then scored
    by diffusion on the database's kNN graph (a dataset with a query set of its own; the same dict comes back).  With a
    `trunc` among them the scores are ranking.diffuse_truncated_device's dense form, and a self-set dataset is accepted."""
    if expand not in EXPAND_ROUTES:
        raise ValueError('expand: one of %s expected, got %r' % (', '.join(EXPAND_ROUTES), expand))
    if diffusion is not None:
        return _eval_diffusion(db, net, trfs, diffusion, detailed, expand,
                               dict(pooling=pooling, gemp=gemp, whiten=whiten, aqe=aqe, adba=adba, threads=threads,
                                    batch_size=batch_size, save_feats=save_feats, load_feats=load_feats))
    if not labelled_on_device(db):
        if expand != 'matrix' and (aqe is not None or adba is not None):
            raise ValueError("expand='lists' needs the device route of a class-labelled dataset "
                             '(DIRTORCH_AMD_DEVICE_RANK=1); test_dir.eval_model expands through the score matrix')
        return test_dir.eval_model(db, net, trfs, pooling=pooling, gemp=gemp, detailed=detailed, whiten=whiten, aqe=aqe,
                                   adba=adba, threads=threads, batch_size=batch_size, save_feats=save_feats,
                                   load_feats=load_feats, dbg=dbg)
    print("\n>> Evaluation...")
    qdescs, bdescs = descriptors(db, net, trfs, pooling=pooling, gemp=gemp, whiten=whiten, aqe=aqe, adba=adba,
                                 threads=threads, batch_size=batch_size, save_feats=save_feats, load_feats=load_feats,
                                 expand=expand)
    aps, tops = ranking.eval_labelled_device(db, qdescs, bdescs)
    res = {}
    test_dir._mean_ap(aps, detailed, res)
    if detailed:
        res['tops'] = tops
    for k in tops[0]:
        res['top%d' % k] = float(np.mean([t[k] for t in tops]))
    return res


def _eval_diffusion(db, net, trfs, diffusion, detailed, expand, desc_kw):
    """eval_model with diffusion scores: descriptors(), ranking.diffuse_device, then the APs on the device where the
    dataset has the revisitop / classic fields and through db.eval_query_AP / eval_query_top on downloaded rows otherwise"""
    same_set = db.get_query_db() is db
    if same_set and not diffusion.get('trunc'):
        raise ValueError('diffusion needs a dataset with a query set of its own: queries that are database rows are '
                         'not supported')
    print("\n>> Evaluation...")
    qdescs, bdescs = descriptors(db, net, trfs, expand=expand, **desc_kw)
    if diffusion.get('trunc'):
        scores = ranking.diffuse_truncated_device(qdescs, bdescs, same_set=same_set, dense=True, **diffusion)
    else:
        scores = ranking.diffuse_device(qdescs, bdescs, **diffusion)
    res = {}
    if hasattr(db, 'junk'):
        test_dir._mean_ap(ranking.eval_aps_device(db, scores), detailed, res)
        return res
    scores = scores.cpu().numpy()
    try:
        test_dir._mean_ap([db.eval_query_AP(q, s) for q, s in enumerate(scores)], detailed, res)
    except NotImplementedError:
        print(" AP not implemented!")
    try:
        tops = [db.eval_query_top(q, s) for q, s in enumerate(scores)]
        if detailed:
            res['tops'] = tops
        for k in tops[0]:
            res['top%d' % k] = float(np.mean([t[k] for t in tops]))
    except NotImplementedError:
        pass
    return res


def main(argv=None):
    """test_dir.main (test_dir.py:194-) around this module's eval_model: same flags, same printout, same json."""
    args = test_dir.build_parser(extra=[
        (('--save-feats',), dict(type=str, default='', help='path to output features')),
        (('--load-feats',), dict(type=str, default='', help='path to load features from')),
        (('--gpu',), dict(type=int, default=0, nargs='+', help='GPU ids')),
        (('--whiten',), dict(type=str, default='Landmarks_clean', help='applies whitening')),
        (('--aqe',), dict(type=int, nargs='+', help='alpha-query expansion paramenters')),
        (('--adba',), dict(type=int, nargs='+', help='alpha-database augmentation paramenters')),
        (('--whitenp',), dict(type=float, default=0.25, help='whitening power, default is 0.5 (i.e., the sqrt)')),
        EXPAND_FLAG,
    ] + DIFFUSION_FLAGS).parse_args(argv)
    iscuda = test_dir.setup_devices(args.gpu)
    qe = {name: (None if val is None else {'k': val[0], 'alpha': val[1]})
          for name, val in (('aqe', args.aqe), ('adba', args.adba))}
    dataset = datasets.create(args.dataset)
    print("Test dataset:", dataset)
    net = test_dir.load_model(args.checkpoint, iscuda)
    whiten = test_dir.select_whitening(net, args)
    res = eval_model(dataset, net, args.trfs, pooling=args.pooling, gemp=args.gemp, detailed=args.detailed,
                     threads=args.threads, dbg=args.dbg, whiten=whiten, aqe=qe['aqe'], adba=qe['adba'],
                     save_feats=args.save_feats, load_feats=args.load_feats, expand=args.expand,
                     diffusion=diffusion_options(args))
    if ddist.rank() == 0:
        print(' * ' + '\n * '.join('%s = %g' % kv for kv in res.items() if np.isscalar(kv[1])))
        if args.out_json:
            try:
                merged = json.load(open(args.out_json))
            except IOError:
                merged = {}
            merged[args.dataset] = res
            mkdir(args.out_json, isfile=True)
            with open(args.out_json, 'w') as f:
                f.write(json.dumps(merged, indent=1))
            print("saved to " + args.out_json)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])

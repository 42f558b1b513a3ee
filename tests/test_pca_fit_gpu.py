"""Fitting a PCA whitening on the MI355X: dir_cov_accumulate (csrc/cov_f32.hip), whitening.PCAFitter, the learn_pca CLI.

  exact     integer-valued X in [-8, 8] and shift in [-3, 3]: |a| <= 11 and N 11^2 < 2^24, so every fp32 chain is exact
            whatever its length and gram / sums must EQUAL the integer reference (fp64 BLAS on integers, exact below 2^53);
  bound     on the generator data of tests/pca_data.py every entry within (R + 3) 2^-24 sum_n |a_ni| |a_nj| of the fp64 sum of
            the same once-rounded operands a = fp32(X - shift), R = dir_cov_chain_rows(): a chain of R fma steps, folded in fp64;
  fit       eigenvalues within the Weyl bound ||C_dev - C64||_2 (+ the LAPACK and fp32-storage terms) of sklearn's fp64 fit;
  scores    the gate that chose R: whitened similarity scores from the device fit are no farther from the fp64 fit's than the
            scores from sklearn's own float32 fit (what a user gets today), and every one of the first D/4 components is at
            least as well aligned with the fp64 fit's;
  CLI       learn_pca on a synthetic checkpoint and image list, then test_dir --whiten KEY on its output.
"""
import os
import pickle

import numpy as np
import pytest
import torch

import pca_data as G

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24


def accumulate(X, shift, gram=None, sums=None):
    from dirtorch_amd import ops
    D = X.shape[1]
    gram = torch.zeros(D, D, dtype=torch.float64, device='cuda') if gram is None else gram
    sums = torch.zeros(D, dtype=torch.float64, device='cuda') if sums is None else sums
    ops.cov_accumulate(X, shift, gram, sums)
    return gram, sums


def integer_case(N, D, ldx, seed, offset=0):
    """X [N, D] as a view with row pitch ldx (the padding columns hold 1e30: they must not be read into anything), base
    moved by `offset` floats; shift; the integer reference in fp64."""
    g = torch.Generator().manual_seed(seed)
    vals = torch.randint(-8, 9, (N, D), generator=g).float()
    shift = torch.randint(-3, 4, (D,), generator=g).float()
    flat = torch.full((N * ldx + offset,), 1e30)
    buf = flat[offset:].view(N, ldx)
    buf[:, :D] = vals
    X = flat.cuda()[offset:].view(N, ldx)[:, :D]
    a = (vals - shift).double().numpy()
    assert np.abs(a).max() <= 11 and N * 11 ** 2 < 2 ** 24
    return X, shift.cuda(), torch.from_numpy(a.T @ a), torch.from_numpy(a.sum(axis=0))


EXACT = [(1, 4, 4, 0), (130, 36, 36, 0), (257, 200, 208, 0), (3001, 131, 131, 0), (5000, 2048, 2048, 0), (70001, 256, 256, 0),
         (130, 36, 40, 1)]     # (the last: a base that is not 16-byte aligned takes the gather path too)


@pytest.mark.parametrize('N,D,ldx,offset', EXACT, ids=['%dx%d_ld%d%s' % (c[0], c[1], c[2], '_off1' if c[3] else '') for c in EXACT])
def test_gram_and_sums_equal_the_integer_reference(N, D, ldx, offset):
    X, shift, gram_ref, sums_ref = integer_case(N, D, ldx, 100 + N, offset)
    assert X.stride(0) == ldx and X.data_ptr() % 16 == (4 * offset) % 16
    gram, sums = accumulate(X, shift)
    assert torch.equal(gram.cpu(), gram_ref) and torch.equal(sums.cpu(), sums_ref)
    assert torch.equal(gram, gram.t())
    # into non-zero accumulators: the call adds
    accumulate(X, shift, gram, sums)
    assert torch.equal(gram.cpu(), 2 * gram_ref) and torch.equal(sums.cpu(), 2 * sums_ref)


def test_no_rows_leave_the_accumulators_untouched():
    D = 36
    gram = torch.full((D, D), 7.0, dtype=torch.float64, device='cuda')
    sums = torch.full((D,), -3.0, dtype=torch.float64, device='cuda')
    accumulate(torch.empty(0, D, device='cuda'), torch.ones(D, device='cuda'), gram, sums)
    torch.cuda.synchronize()
    assert bool((gram == 7.0).all()) and bool((sums == -3.0).all())


def test_partial_fit_in_ragged_chunks_equals_one_call():
    """Integer data: every association of the sum is exact, so the split state must equal the one-pass state bit for bit; the
    host-array path (uploaded in pieces) and the device-tensor path feed the same kernel."""
    from dirtorch_amd import whitening
    X, shift, gram_ref, sums_ref = integer_case(3001, 131, 131, 5)
    Xh, sh = X.cpu().numpy(), shift.cpu().numpy()
    one = whitening.PCAFitter(131, shift=sh).partial_fit(X).state()
    two = whitening.PCAFitter(131, shift=sh).partial_fit(X[:1237]).partial_fit(Xh[1237:]).state()
    assert one['n'] == two['n'] == 3001
    for k in ('gram', 'sums', 'shift'):
        assert np.array_equal(one[k], two[k]), k
    assert np.array_equal(one['gram'], gram_ref.numpy()) and np.array_equal(one['sums'], sums_ref.numpy())
    # merge of two device-fed halves; from_state continues on the device
    a = whitening.PCAFitter(131, shift=sh).partial_fit(X[:1237])
    b = whitening.PCAFitter(131, shift=sh).partial_fit(X[1237:])
    assert np.array_equal(a.merge(b).state()['gram'], one['gram'])
    c = whitening.PCAFitter.from_state(whitening.PCAFitter(131, shift=sh).partial_fit(X[:1237]).state()).partial_fit(X[1237:])
    assert np.array_equal(c.state()['gram'], one['gram']) and c.n == 3001
    # no shift given: the fp64 mean of the first chunk's first <= 4096 rows, rounded to fp32
    assert np.array_equal(whitening.PCAFitter(131).partial_fit(X).state()['shift'], G.default_shift(Xh))


class Fit(object):
    pass


def _fit(N, D, ldx, seed):
    from dirtorch_amd import ops, whitening
    from sklearn.decomposition import PCA
    f = Fit()
    f.X = G.descriptors(N, D, seed)
    f.shift = G.default_shift(f.X)
    buf = torch.zeros(N, ldx, device='cuda')
    buf[:, :D] = torch.from_numpy(f.X).cuda()
    f.Xd = buf[:, :D] if ldx != D else buf
    f.R = ops.cov_chain_rows()
    fitter = whitening.PCAFitter(D).partial_fit(f.Xd)
    f.state = fitter.state()
    f.pca = fitter.finalize()
    f.ref = G.state64(f.X, f.shift)
    f.sk64 = G.sklearn_fit64(f.X, whiten=True)
    f.sk32 = PCA(svd_solver='full', whiten=True).fit(f.X)        # sklearn's own float32 fit: what a user gets today
    return f


@pytest.fixture(scope='module', params=[(6000, 256, 256, 21), (3000, 192, 200, 22)], ids=['6000x256', '3000x192_ld200'])
def fit(request):
    """One device fit and its references per data set; shared by the tests below, never modified."""
    return _fit(*request.param)


def test_every_gram_entry_is_within_the_chain_bound(fit):
    f = fit
    assert np.array_equal(f.state['shift'], f.shift) and f.state['n'] == len(f.X)
    a = np.abs(G.shifted(f.X, f.shift))
    bound = (f.R + 3) * U32 * (a.T @ a)
    err = np.abs(f.state['gram'] - f.ref['gram'])
    sbound = (f.R + 3) * U32 * a.sum(axis=0)
    serr = np.abs(f.state['sums'] - f.ref['sums'])
    print('\n[pca-fit] %d x %d, R = %d: max |gram - gram64| / bound = %.4f (max abs %.3e), sums %.4f'
          % (f.X.shape + (f.R, (err / bound).max(), err.max(), (serr / sbound).max())))
    assert np.all(err <= bound) and np.all(serr <= sbound)
    assert np.array_equal(f.state['gram'], f.state['gram'].T)
    # run-to-run identical: no atomics, fixed reduction order
    from dirtorch_amd import whitening
    again = whitening.PCAFitter(f.X.shape[1]).partial_fit(f.Xd).state()
    assert np.array_equal(again['gram'], f.state['gram']) and np.array_equal(again['sums'], f.state['sums'])


def test_fit_eigenvalues_within_the_weyl_bound_of_the_fp64_fit(fit):
    f = fit
    D = f.X.shape[1]
    C64 = np.cov(f.X.astype(np.float64), rowvar=False)
    weyl = np.linalg.norm(G.covariance(f.state) - C64, 2)
    lam64 = f.sk64.explained_variance_
    bound = weyl + G.lapack_term(D, lam64[0]) + U32 * lam64          # (+ explained_variance_ is stored in fp32)
    err = np.abs(f.pca.explained_variance_.astype(np.float64) - lam64)
    err32 = np.abs(f.sk32.explained_variance_.astype(np.float64) - lam64)
    print('\n[pca-fit] %d x %d: ||C_dev - C64||_2 = %.3e (lambda_max %.3e, lambda_min %.3e); max eigenvalue error: device fit '
          '%.3e, sklearn float32 fit %.3e' % (f.X.shape + (weyl, lam64[0], lam64[-1], err.max(), err32.max())))
    assert np.all(err <= bound), (err / bound).max()
    mean64 = f.X.astype(np.float64).mean(axis=0)
    assert np.all(np.abs(f.pca.mean_.astype(np.float64) - mean64) <= U32 * np.abs(mean64) + 1e-12)


def _scores(pca, Q, B, whitenp):
    """Whitened similarity scores in fp64 from a fit's stored attributes: only the fits differ between two calls."""
    import dir_oracle as O
    P = O.PCAParams(np.asarray(pca.mean_, np.float64), np.asarray(pca.components_, np.float64),
                    np.asarray(pca.explained_variance_, np.float64), True)
    q = O.whiten_features(Q.astype(np.float64), P, whitenp=whitenp)
    b = O.whiten_features(B.astype(np.float64), P, whitenp=whitenp)
    return q @ b.T


def _alignment(pca, ref, k):
    """|cos| between each of the first k components and the fp64 fit's.  The stored vectors are unit vectors up to their fp32
    rounding; normalising them takes that storage artefact (a change of LENGTH of ~1e-8, either way) out of the comparison."""
    v = np.asarray(pca.components_[:k], np.float64)
    w = np.asarray(ref.components_[:k], np.float64)
    return np.abs(np.sum(v * w, axis=1)) / (np.linalg.norm(v, axis=1) * np.linalg.norm(w, axis=1))


@pytest.mark.parametrize('whitenp', [0.25, 0.5])
def test_scores_from_the_device_fit_are_no_farther_from_fp64_than_sklearns_float32_fit(fit, whitenp):
    f = fit
    D = f.X.shape[1]
    Q, B = f.X[:64], f.X[64:2064]
    s64 = _scores(f.sk64, Q, B, whitenp)
    d_dev = np.abs(_scores(f.pca, Q, B, whitenp) - s64).max()
    d_32 = np.abs(_scores(f.sk32, Q, B, whitenp) - s64).max()
    a_dev, a_32 = _alignment(f.pca, f.sk64, D // 4), _alignment(f.sk32, f.sk64, D // 4)
    worse = np.flatnonzero(a_dev < a_32)
    print('\n[pca-fit] %d x %d, whitenp %.2f, R = %d: score distance from the fp64 fit: device fit %.3e, sklearn float32 fit %.3e; '
          'first D/4 components, max 1 - |cos|: device %.3e, float32 %.3e; components less aligned than float32: %d'
          % (f.X.shape + (whitenp, f.R, d_dev, d_32, (1 - a_dev).max(), (1 - a_32).max(), len(worse))))
    assert d_dev <= d_32, (d_dev, d_32)
    assert len(worse) == 0, [(int(i), float(1 - a_dev[i]), float(1 - a_32[i])) for i in worse[:8]]


def _save_images(root, names, sizes, seed):
    from PIL import Image
    r = np.random.RandomState(seed)
    os.makedirs(root, exist_ok=True)
    for name, (h, w) in zip(names, sizes):
        yy, xx = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing='ij')
        img = np.stack([127 + 100 * np.sin(r.uniform(2, 9) * yy * 6.28 + r.uniform(0, 6)) * np.cos(r.uniform(2, 9) * xx * 6.28)
                        + 20 * r.standard_normal((h, w)) for _ in range(3)], -1)
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(root, name))


def test_learn_pca_cli_then_test_dir_whiten(tmp_path, monkeypatch):
    """python -m dirtorch_amd.learn_pca on a synthetic ResNet-18 checkpoint and a revisitop-format image set, then
    test_dir --whiten KEY and extract_features --whiten KEY on the checkpoint it wrote."""
    import dir_oracle as O
    from dirtorch_amd import extract_features as ef, learn_pca, test_dir as td, whitening
    from dirtorch_amd.utils import common
    root = tmp_path / 'oxford5k'
    N, Q, D = 12, 2, 128
    r = np.random.RandomState(8)
    names = ['im%02d' % i for i in range(N)]
    sizes = [(int(r.randint(64, 97)), int(r.randint(64, 97))) for _ in range(N)]
    _save_images(str(root / 'jpg'), [n + '.jpg' for n in names], sizes, 4)
    gnd = [{'bbx': [2, 3, sizes[q][1] - 3, sizes[q][0] - 2], 'easy': [2 + 2 * q], 'hard': [3 + 2 * q], 'junk': [q]} for q in range(Q)]
    with open(str(root / 'gnd_roxford5k.pkl'), 'wb') as fh:
        pickle.dump({'imlist': names, 'qimlist': names[:Q], 'gnd': gnd}, fh)
    (tmp_path / 'list.txt').write_text('\n'.join(n + '.jpg' for n in names) + '\n')
    monkeypatch.setenv('DB_ROOT', str(tmp_path))
    sd = O.synth_state_dict('resnet18', seed=7, gemp=3.0, out_dim=D)
    old = whitening.PCAFitter.from_state(G.state64(G.descriptors(40, D, 1), np.zeros(D, np.float32))).finalize(n_components=4)
    ck_in, ck_out = str(tmp_path / 'in.pt'), str(tmp_path / 'out' / 'with_pca.pt')
    torch.save({'model_options': dict(arch='resnet18_rmac', out_dim=D, pooling='gem', gemp=3),
                'state_dict': {'module.' + k: v for k, v in sd.items()}, 'pca': {'Landmarks_clean': old}, 'epoch': 3}, ck_in)
    listed = 'ImageList("%s", root="%s")' % (tmp_path / 'list.txt', root / 'jpg')
    learn_pca.main(['--dataset', listed, '--checkpoint', ck_in, '--output', ck_out, '--name', 'mine', '--gpu', '0', '--threads', '0'])
    ck = common.torch_load_trusted(ck_out)
    assert ck['epoch'] == 3 and set(ck['pca']) == {'Landmarks_clean', 'mine'} and ck['model_options']['out_dim'] == D
    assert all(k.startswith('module.') for k in ck['state_dict']) and len(ck['state_dict']) == len(sd)
    assert np.array_equal(ck['pca']['Landmarks_clean'].components_, old.components_)
    mine = ck['pca']['mine']
    assert mine.components_.shape == (N, D) and mine.n_samples_ == N and mine.components_.dtype == np.float32
    # the evaluation runs on it unchanged
    res = td.main(['--dataset', 'ROxford5K', '--checkpoint', ck_out, '--gpu', '0', '--threads', '0', '--whiten', 'mine',
                   '--whitenp', '0.5', '--whitenv', '8', '--save-feats', str(tmp_path / 'feats')])
    assert all(np.isfinite(res[k]) for k in ('mAP-easy', 'mAP-medium', 'mAP-hard'))
    # ... and what it whitens with is a PCAFitter fit of the same extracted descriptors (--save-feats keeps the database
    # descriptors as they are before whitening: the same files in the same order as the list the PCA was learnt on)
    wh = str(tmp_path / 'wh.npy')
    ef.main(['--dataset', listed, '--checkpoint', ck_out, '--output', wh, '--gpu', '0', '--threads', '0', '--whiten', 'mine',
             '--whitenp', '0.5', '--whitenv', '8'])
    descs = np.load(str(tmp_path / 'feats' / 'feats.bdescs.npy'))
    assert descs.shape == (N, D) and descs.dtype == np.float32
    refit = whitening.PCAFitter(D).partial_fit(descs).finalize()
    assert np.array_equal(refit.components_, mine.components_) and np.array_equal(refit.mean_, mine.mean_)
    expect = common.whiten_features(descs, refit, whitenp=0.5, whitenv=8)
    got = np.load(wh)
    assert got.shape == (N, 8) and np.isfinite(got).all() and np.array_equal(got, expect)
    # a default --name is the dataset command
    learn_pca.main(['--dataset', listed, '--checkpoint', ck_out, '--output', ck_out, '--gpu', '0', '--threads', '0', '--max-images', '9'])
    again = common.torch_load_trusted(ck_out)['pca']
    assert set(again) == {'Landmarks_clean', 'mine', listed} and again[listed].n_samples_ == 9

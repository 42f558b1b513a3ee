"""The host half of the PCA fit (dirtorch_amd/whitening.py) and the argument checks of dir_cov_accumulate: no GPU.

States are built in numpy fp64 (tests/pca_data.py) - what the device accumulates is tested in tests/test_pca_fit_gpu.py -
and finalize() is held against sklearn's PCA(svd_solver='full') on the fp64 data:
  * means to fp32 rounding (mean_ is stored in fp32 as in the reference's checkpoints);
  * every eigenvalue within the Weyl bound ||C - C64||_2 of the two covariance matrices, plus 64 D 2^-53 lambda_max for the
    two LAPACK calls, plus 2^-24 lambda_i for the fp32 storage of explained_variance_;
  * sklearn's sign rule, descending order.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import pca_data as G

U32 = 2.0 ** -24


@pytest.fixture(scope='module')
def fitted():
    """(X, state, PCA from finalize, sklearn's fp64 fit) of one 700 x 96 set; shared, never modified."""
    from dirtorch_amd import whitening
    X = G.descriptors(700, 96, 11)
    st = G.state64(X, G.default_shift(X))
    pca = whitening.PCAFitter.from_state(st).finalize()
    return X, st, pca, G.sklearn_fit64(X, whiten=True)


def test_finalize_matches_sklearn_full_svd_on_fp64_data(fitted):
    X, st, pca, ref = fitted
    D = X.shape[1]
    X64 = X.astype(np.float64)
    mean64 = X64.mean(axis=0)
    assert pca.mean_.dtype == pca.components_.dtype == pca.explained_variance_.dtype == np.float32
    assert np.all(np.abs(pca.mean_.astype(np.float64) - mean64) <= U32 * np.abs(mean64) + 1e-15)
    C64 = np.cov(X64, rowvar=False)
    weyl = np.linalg.norm(G.covariance(st) - C64, 2)
    lam64 = ref.explained_variance_
    bound = weyl + G.lapack_term(D, lam64[0]) + U32 * lam64
    err = np.abs(pca.explained_variance_.astype(np.float64) - lam64)
    print('\n[pca-fit-cpu] max eigenvalue error %.3e, smallest bound %.3e (Weyl %.3e)' % (err.max(), bound.min(), weyl))
    assert np.all(err <= bound), (err.max(), bound.min())
    ev = pca.explained_variance_
    assert np.all(ev[:-1] >= ev[1:]) and np.all(ev >= 0)
    big = np.argmax(np.abs(pca.components_), axis=1)
    assert np.all(pca.components_[np.arange(len(big)), big] > 0)
    # well-separated leading directions are sklearn's, sign included
    lead = np.abs(np.sum(pca.components_[:8].astype(np.float64) * ref.components_[:8], axis=1))
    assert np.all(lead > 1 - 1e-6) and np.all(np.sum(pca.components_[:8] * ref.components_[:8], axis=1) > 0)
    # the bookkeeping attributes of a fitted sklearn PCA
    assert pca.n_components_ == D and pca.n_samples_ == 700 and pca.n_features_in_ == D and pca.whiten is True
    assert pca.noise_variance_ == 0.0
    np.testing.assert_allclose(pca.explained_variance_ratio_, ref.explained_variance_ratio_, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(pca.singular_values_, ref.singular_values_, rtol=1e-5, atol=1e-7)
    from sklearn.decomposition import PCA
    assert isinstance(pca, PCA)
    # ... a real one: sklearn's own transform runs on it and agrees with the fp64 fit's on the leading directions
    t, t_ref = pca.transform(X[:5])[:, :8], ref.transform(X64[:5])[:, :8]
    assert np.abs(t - t_ref).max() < 1e-4 * np.abs(t_ref).max()


def test_state_is_additive_and_merge_checks_the_shift():
    from dirtorch_amd import whitening
    r = np.random.RandomState(3)
    X = r.randint(-8, 9, size=(301, 40)).astype(np.float32)
    shift = r.randint(-3, 4, size=40).astype(np.float32)
    whole = whitening.PCAFitter.from_state(G.state64(X, shift))
    a = whitening.PCAFitter.from_state(G.state64(X[:117], shift))
    b = whitening.PCAFitter.from_state(G.state64(X[117:], shift))
    m, w = a.merge(b).state(), whole.state()
    assert m['n'] == w['n'] == 301
    assert np.array_equal(m['gram'], w['gram']) and np.array_equal(m['sums'], w['sums'])
    assert np.array_equal(m['shift'], shift) and m['shift'].dtype == np.float32
    assert m['gram'].dtype == m['sums'].dtype == np.float64
    with pytest.raises(ValueError):
        a.merge(whitening.PCAFitter.from_state(G.state64(X[:50], shift + 1)))
    with pytest.raises(ValueError):
        a.merge(whitening.PCAFitter(41))
    # an empty fitter adopts the other's shift; state() hands out copies
    e = whitening.PCAFitter(40).merge(whole)
    assert np.array_equal(e.state()['gram'], w['gram']) and e.state()['n'] == 301
    w['gram'][0, 0] += 1
    assert whole.state()['gram'][0, 0] == w['gram'][0, 0] - 1
    assert whitening.PCAFitter(40).state()['shift'] is None and whitening.PCAFitter(40).state()['n'] == 0


def test_n_components_truncates_and_small_n_raises(fitted):
    from dirtorch_amd import whitening
    X, st, full, _ = fitted
    f = whitening.PCAFitter.from_state(st)
    p = f.finalize(n_components=10, whiten=False)
    assert p.components_.shape == (10, 96) and p.explained_variance_.shape == (10,) and p.n_components_ == 10
    assert p.whiten is False and p.mean_.shape == (96,)
    assert np.array_equal(p.components_, full.components_[:10]) and np.array_equal(p.explained_variance_, full.explained_variance_[:10])
    assert abs(p.noise_variance_ - float(full.explained_variance_[10:].astype(np.float64).mean())) < 1e-6 * p.noise_variance_
    for bad in (0, 97):
        with pytest.raises(ValueError):
            f.finalize(n_components=bad)
    with pytest.raises(ValueError):
        whitening.PCAFitter(8).finalize()
    with pytest.raises(ValueError):
        whitening.PCAFitter.from_state(G.state64(X[:1, :8], np.zeros(8, np.float32))).finalize()
    # fewer samples than dimensions: min(n, D) components, as sklearn's full solver
    few = whitening.PCAFitter.from_state(G.state64(X[:20], G.default_shift(X[:20]))).finalize()
    assert few.components_.shape == (20, 96)


def test_fitted_pca_survives_a_checkpoint_round_trip(tmp_path, fitted):
    from dirtorch_amd.utils import common
    _, _, pca, _ = fitted
    path = str(tmp_path / 'ck.pt')
    torch.save({'model_options': {'arch': 'resnet18_rmac'}, 'state_dict': {'w': torch.zeros(2)}, 'pca': {'mine': pca}}, path)
    back = common.torch_load_trusted(path)['pca']['mine']
    assert type(back) is type(pca)
    for name in ('mean_', 'components_', 'explained_variance_', 'explained_variance_ratio_', 'singular_values_'):
        assert np.array_equal(getattr(back, name), getattr(pca, name)) and getattr(back, name).dtype == np.float32, name
    assert back.whiten is True and back.n_components_ == pca.n_components_ and back.n_samples_ == 700


def test_the_attributes_common_transform_reads_and_to_dict(fitted):
    """common.transform (dirtorch/utils/common.py:221-232) reads mean_, components_[:v], explained_variance_[:v] and whiten:
    the oracle's restatement of it runs on the returned object, and to_dict's {'W', 'means'} reproduces it through the
    use_sklearn=False formula (X - means) W.  W is stored in fp32: each output may differ from the fp64 formula by
    2^-24 sum_k |x_k - m_k| |W_kj|, the rounding of W's entries."""
    import dir_oracle as O
    from dirtorch_amd import whitening
    X, _, pca, _ = fitted
    X64 = X[:64].astype(np.float64)
    for whitenp, whitenv, whitenm in ((0.5, None, 1.0), (0.25, 32, 2.0)):
        P64 = O.PCAParams(pca.mean_.astype(np.float64), pca.components_.astype(np.float64),
                          pca.explained_variance_.astype(np.float64), pca.whiten)
        ref = O.whiten_features(X64, P64, l2norm=False, whitenp=whitenp, whitenv=whitenv, whitenm=whitenm)
        same = O.whiten_features(X64, pca, l2norm=False, whitenp=whitenp, whitenv=whitenv, whitenm=whitenm)   # the object itself
        assert same.shape == ref.shape and np.abs(same - ref).max() <= 1e-5 * np.abs(ref).max()
        d = whitening.to_dict(pca, whitenp, whitenv, whitenm)
        assert d['W'].dtype == d['means'].dtype == np.float32 and d['W'].shape == (96, whitenv or 96)
        xm = X64 - d['means'].astype(np.float64)
        got = xm @ d['W'].astype(np.float64)
        bound = U32 * (np.abs(xm) @ np.abs(d['W'].astype(np.float64))) * 1.01 + 1e-15
        assert np.all(np.abs(got - ref) <= bound), (np.abs(got - ref) / bound).max()
    plain = O.PCAParams(pca.mean_, pca.components_, pca.explained_variance_, False)
    assert np.array_equal(whitening.to_dict(plain, 0.5, 16, 1.0)['W'], np.ascontiguousarray(pca.components_[:16].T))


def test_partial_fit_rejects_what_it_cannot_add():
    from dirtorch_amd import whitening
    f = whitening.PCAFitter(8)
    with pytest.raises(ValueError):
        f.partial_fit(np.zeros((4, 9), np.float32))
    with pytest.raises(TypeError):
        f.partial_fit(np.zeros((4, 8), np.float64))
    with pytest.raises(ValueError):
        whitening.PCAFitter(8, shift=np.zeros(7, np.float32))
    assert f.partial_fit(np.zeros((0, 8), np.float32)).state()['n'] == 0      # an empty chunk: nothing to launch


def test_cov_accumulate_argument_errors_do_not_need_a_gpu():
    from dirtorch_amd import _lib, ops
    lib = _lib.load()
    R = lib.dir_cov_chain_rows()
    assert R >= 1 and ops.cov_chain_rows() == R
    x = (ctypes.c_float * 64)()
    s = (ctypes.c_float * 8)()
    g = (ctypes.c_double * 64)()
    m = (ctypes.c_double * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    for args, word in (((None, 8, 4, 8, p(s), p(g), p(m)), b'null'), ((p(x), 8, 4, 8, None, p(g), p(m)), b'null'),
                       ((p(x), 8, 4, 8, p(s), None, p(m)), b'null'), ((p(x), 8, 4, 8, p(s), p(g), None), b'null'),
                       ((p(x), 7, 4, 8, p(s), p(g), p(m)), b'ldx'), ((p(x), 8, -1, 8, p(s), p(g), p(m)), b'N must'),
                       ((p(x), 8, 4, 0, p(s), p(g), p(m)), b'D >= 1'), ((p(x), 8, 0, 8, None, p(g), p(m)), b'null')):
        assert lib.dir_cov_accumulate(*args, None) == -1, args
        assert word in lib.dir_last_error(), (args, lib.dir_last_error())
    with pytest.raises(_lib.DirError):
        _lib.call('dir_cov_accumulate', None, 8, 4, 8, None, None, None, None)
    assert lib.dir_cov_accumulate(p(x), 8, 0, 8, p(s), p(g), p(m), None) == 0      # N = 0: nothing to do, nothing touched
    assert lib.dir_cov_accumulate(None, 8, 0, 8, p(s), p(g), p(m), None) == 0      # (an empty X has no address)
    assert not any(g) and not any(m)


def test_learn_pca_cli_is_importable_and_documents_its_flags():
    from dirtorch_amd import learn_pca
    with pytest.raises(SystemExit):
        learn_pca.main(['--help'])
    integration = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'INTEGRATION.md')).read()
    for flag in ('--dataset', '--checkpoint', '--output', '--name', '--trfs', '--pooling', '--gemp', '--gpu', '--threads', '--max-images'):
        assert flag in integration, flag
    assert 'dirtorch_amd.learn_pca' in integration

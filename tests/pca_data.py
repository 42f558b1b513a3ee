"""Inputs and fp64 references shared by tests/test_pca_fit_cpu.py and tests/test_pca_fit_gpu.py (not a test module).

    descriptors     the generator of the PCA-fit tests: rows z * logspace(0, -2, D) (four decades of variance) rotated by a
                    random orthogonal matrix, plus a common positive offset (the strong common mean of L2-normalised
                    all-positive descriptors), L2-normalised, cast to fp32
    state64         the state {'gram', 'sums', 'n', 'shift'} of whitening.PCAFitter in numpy fp64
    lapack_term     what two LAPACK eigen-decompositions of D x D matrices may differ by: 64 D 2^-53 lambda_max
"""
import numpy as np

OFFSET = 0.5      # per coordinate, against a noise row norm of ~0.33 sqrt(D): the common mean carries most of a row's norm


def descriptors(n, D, seed):
    r = np.random.RandomState(seed)
    z = r.standard_normal((n, D)) * np.logspace(0, -2, D)
    q, _ = np.linalg.qr(r.standard_normal((D, D)))
    x = z @ q + OFFSET
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.ascontiguousarray(x.astype(np.float32))


def default_shift(X):
    """What PCAFitter picks when no shift is given: the fp64 column mean of the first <= 4096 rows, rounded to fp32."""
    return X[:4096].astype(np.float64).mean(axis=0).astype(np.float32)


def shifted(X, shift):
    """a = X - shift as the kernel forms it: one fp32 subtraction per entry; returned in fp64."""
    return (X.astype(np.float32) - shift.astype(np.float32)[None, :]).astype(np.float64)


def state64(X, shift):
    a = shifted(X, shift)
    return {'gram': a.T @ a, 'sums': a.sum(axis=0), 'n': int(X.shape[0]), 'shift': shift.astype(np.float32)}


def covariance(state):
    """finalize()'s covariance, restated."""
    n, s = state['n'], state['sums']
    return (state['gram'] - np.outer(s, s) / n) / (n - 1)


def lapack_term(D, lam_max):
    return 64.0 * D * 2.0 ** -53 * lam_max


def sklearn_fit64(X, **kw):
    from sklearn.decomposition import PCA
    return PCA(svd_solver='full', **kw).fit(X.astype(np.float64))

"""Learning a PCA whitening - the side of dirtorch/utils/common.py:221-239 the reference leaves to the user.

The reference applies a pickled sklearn.decomposition.PCA (ck['pca'][NAME]) and ships the Landmarks18_pca image list to fit
one on, but no code for the fit.  Here the fit is split where its cost splits:

    on the device   everything that depends on the number of descriptors N: the shifted Gram matrix and the column sums,
                    gram += (X - shift)^T (X - shift),  sums += sum_n (X[n] - shift)      (ops.cov_accumulate, csrc/cov_f32.hip)
                    in fp64 accumulators fed by bounded fp32 MFMA chains, in as many chunks as the descriptors come in;
    on the host     the D x D steps, O(D^3) and independent of N, in numpy fp64: merging two states, and finalize() -
                    mean = shift + sums / n,  C = (gram - sums sums^T / n) / (n - 1),  numpy.linalg.eigh(C).
                    This is the one place the package does arithmetic on the CPU, on purpose: it is the same kind of step as
                    the `alpha` vector common._transform_dev builds on the host, and no part of it grows with the data.

`shift` is a choice of origin, not part of the result: any value gives the same covariance in exact arithmetic, one close to
the column mean keeps the sums sums^T / n correction tiny so that nothing cancels (L2-normalised descriptors have a strong
common mean).  When none is given the host takes it from the first <= 4096 rows it sees.

The state {'gram', 'sums', 'n', 'shift'} is additive for a fixed shift: PCAFitter.merge adds two of them, so a multi-rank
fit is one all-reduce of D^2 + D doubles (33 MB at D = 2048) instead of a gather of N x D descriptors.
"""
import numpy as np

SHIFT_ROWS = 4096            # rows of the first chunk the default shift is the mean of
UPLOAD_BYTES = 256 << 20     # host arrays go to the device in pieces of at most this size


class PCAParams(object):
    """The four attributes common.transform reads (common.py:224-228) - what finalize() returns when scikit-learn cannot be
    imported."""

    def __init__(self, mean_, components_, explained_variance_, whiten=True):
        self.mean_ = mean_
        self.components_ = components_
        self.explained_variance_ = explained_variance_
        self.whiten = whiten


def _is_tensor(x):
    return type(x).__module__ == 'torch'


class PCAFitter(object):
    """Streaming PCA fit of D-dimensional fp32 descriptors: partial_fit(X) any number of times, then finalize()."""

    def __init__(self, D, shift=None):
        self.D = int(D)
        if self.D < 1:
            raise ValueError('D must be >= 1')
        self.n = 0
        self.shift = None if shift is None else self._check_shift(shift)
        self._host = (np.zeros((self.D, self.D), np.float64), np.zeros(self.D, np.float64))
        self._dev = None         # (gram, sums, shift) CUDA tensors once partial_fit has run; then they hold the state

    def _check_shift(self, shift):
        shift = np.ascontiguousarray(shift, dtype=np.float32).reshape(-1).copy()
        if shift.shape != (self.D,):
            raise ValueError('shift must have D = %d entries' % self.D)
        return shift

    # ---- the N-dependent half: device ---------------------------------------------------------------------------------
    def _device_state(self):
        import torch
        if self._dev is None:
            self._dev = (torch.from_numpy(self._host[0]).cuda(), torch.from_numpy(self._host[1]).cuda(),
                         torch.from_numpy(self.shift).cuda())
            self._host = None
        return self._dev

    def partial_fit(self, X):
        """Add the rows of X [n, D] - an fp32 ndarray or an fp32 CUDA tensor - to the state."""
        import torch
        from . import ops
        tensor = _is_tensor(X)
        if X.ndim != 2 or X.shape[1] != self.D:
            raise ValueError('X must be [n, %d], got %s' % (self.D, tuple(X.shape)))
        if (X.dtype != torch.float32) if tensor else (X.dtype != np.float32):
            raise TypeError('float32 descriptors expected, got %s' % X.dtype)
        if tensor and not X.is_cuda:
            X, tensor = X.numpy(), False
        n = int(X.shape[0])
        if n == 0:
            return self
        if self.shift is None:
            head = X[:SHIFT_ROWS]
            head = head.cpu().numpy() if tensor else np.asarray(head)
            self.shift = head.astype(np.float64).mean(axis=0).astype(np.float32)
        gram, sums, shift = self._device_state()
        if tensor:
            ops.cov_accumulate(X, shift, gram, sums)
        else:
            rows = max(1, UPLOAD_BYTES // (4 * self.D))
            for r in range(0, n, rows):
                piece = torch.from_numpy(np.ascontiguousarray(X[r:r + rows])).cuda()
                ops.cov_accumulate(piece, shift, gram, sums)
        self.n += n
        return self

    # ---- the state ----------------------------------------------------------------------------------------------------
    def state(self):
        """{'gram' [D,D] fp64, 'sums' [D] fp64, 'n' int, 'shift' [D] fp32 or None when no row has been seen}: copies."""
        if self._dev is not None:
            gram, sums = self._dev[0].cpu().numpy(), self._dev[1].cpu().numpy()
        else:
            gram, sums = self._host[0].copy(), self._host[1].copy()
        return {'gram': gram, 'sums': sums, 'n': int(self.n), 'shift': None if self.shift is None else self.shift.copy()}

    @classmethod
    def from_state(cls, state):
        gram = np.array(state['gram'], dtype=np.float64)
        D = gram.shape[0]
        sums = np.array(state['sums'], dtype=np.float64).reshape(-1)
        if gram.shape != (D, D) or sums.shape != (D,):
            raise ValueError('state: gram [D,D] and sums [D] expected')
        f = cls(D, shift=state['shift'])
        f.n = int(state['n'])
        if f.n < 0 or (f.n > 0 and f.shift is None):
            raise ValueError('state: n >= 0, and a shift once rows have been added')
        f._host = (gram, sums)
        return f

    def merge(self, other):
        """Add another fitter's state (same D, IDENTICAL shift) to this one; a D x D host step."""
        if other.D != self.D:
            raise ValueError('merge: D differs (%d, %d)' % (self.D, other.D))
        if other.n == 0:
            return self
        if self.n == 0 and self.shift is None:
            self.shift = other.shift.copy()
        if not np.array_equal(self.shift, other.shift):
            raise ValueError('merge: the two states were accumulated around different shifts')
        a, b = self.state(), other.state()
        self._dev = None
        self._host = (a['gram'] + b['gram'], a['sums'] + b['sums'])
        self.n = a['n'] + b['n']
        return self

    # ---- the D x D half: host, numpy fp64 -----------------------------------------------------------------------------
    def finalize(self, n_components=None, whiten=True):
        """The PCA of everything added so far: a sklearn.decomposition.PCA with its fitted attributes set (mean_, components_
        and explained_variance_ fp32 as in the reference's checkpoints), whose pickle loads wherever theirs does."""
        st = self.state()
        n, D = st['n'], self.D
        if n < 2:
            raise ValueError('a PCA needs at least 2 samples, got %d' % n)
        gram, sums = st['gram'], st['sums']
        mean = st['shift'].astype(np.float64) + sums / n
        C = (gram - np.outer(sums, sums) / n) / (n - 1)
        w, V = np.linalg.eigh(C)
        w, V = np.maximum(w[::-1], 0.0), V[:, ::-1]                  # descending; rounding can leave tiny negatives
        comps = np.ascontiguousarray(V.T)
        # sklearn's sign rule (svd_flip on the rows of V^T): each component's largest-magnitude entry is positive
        big = np.argmax(np.abs(comps), axis=1)
        comps *= np.where(comps[np.arange(D), big] < 0, -1.0, 1.0)[:, None]
        kmax = min(n, D)
        k = kmax if n_components is None else int(n_components)
        if not 1 <= k <= kmax:
            raise ValueError('n_components=%r must be between 1 and min(n, D) = %d' % (n_components, kmax))
        total = w.sum()
        noise = float(w[k:kmax].mean()) if k < kmax else 0.0
        f32 = np.float32
        attrs = dict(mean_=mean.astype(f32), components_=comps[:k].astype(f32), explained_variance_=w[:k].astype(f32),
                     explained_variance_ratio_=(w[:k] / total if total > 0 else np.zeros(k)).astype(f32),
                     singular_values_=np.sqrt(w[:k] * (n - 1)).astype(f32), n_components_=k, n_samples_=n,
                     n_features_in_=D, noise_variance_=noise)
        try:
            from sklearn.decomposition import PCA
        except ImportError:
            return PCAParams(attrs['mean_'], attrs['components_'], attrs['explained_variance_'], bool(whiten))
        pca = PCA(n_components=k, whiten=bool(whiten), svd_solver='full')
        for name, val in attrs.items():
            setattr(pca, name, val)
        return pca


def fit_pca(X, shift=None, n_components=None, whiten=True):
    """The whole fit in one call: X [N, D] fp32 ndarray or CUDA tensor -> fitted PCA (PCAFitter.finalize)."""
    return PCAFitter(X.shape[1], shift=shift).partial_fit(X).finalize(n_components=n_components, whiten=whiten)


def to_dict(pca, whitenp=0.5, whitenv=None, whitenm=1.0):
    """{'W' [D, v], 'means' [D]} for the use_sklearn=False branch of common.transform (common.py:229-231): X_t = (X - means) W,
    the variance scaling 1 / (whitenm * explained_variance^whitenp) folded into the columns of W."""
    W = np.asarray(pca.components_[:whitenv], dtype=np.float64).T
    if pca.whiten:
        W = W / (whitenm * np.power(np.asarray(pca.explained_variance_[:whitenv], dtype=np.float64), whitenp))
    mean = np.zeros(W.shape[0], np.float32) if pca.mean_ is None else np.asarray(pca.mean_, dtype=np.float32)
    return {'W': np.ascontiguousarray(W.astype(np.float32)), 'means': mean}

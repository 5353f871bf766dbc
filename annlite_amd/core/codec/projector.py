"""``ProjectorCodec`` -- the PCA projection of ``AnnLite(n_components=K, projector='gpu')``; mirrors
annlite/core/codec/projector.py:8-156 (signature, ``__hash__``, asserts, properties).

The reference wraps sklearn: ``PCA(n_components, whiten, svd_solver).fit`` (an SVD of the centred data) in ``fit``,
``IncrementalPCA.partial_fit`` (a rank-truncated running SVD) in ``partial_fit``, ``transform`` / ``inverse_transform`` in
``encode`` / ``decode``.  Here, by a different route to the same subspace:

* the data pass of a fit -- ``sum (x - s)`` and ``sum (x - s)(x - s)^T`` about a shift ``s`` near the mean -- runs on the GPU
  (``ops.pca_accumulate``: chunked f32 MFMA products folded into float64 accumulators in a fixed order);
* ``_finalize`` -- plain numpy float64 on the host, once per fit -- turns the sums into the mean, the covariance, its
  eigen-decomposition (``numpy.linalg.eigh``), and sklearn's sign convention;
* ``encode`` / ``decode`` are one GPU kernel (``ops.affine_rows``): ``(x - mean) W^T`` and ``z W + mean``.

``svd_solver`` is kept for the signature and ``__hash__`` only: there is one solver.

``partial_fit`` differs from IncrementalPCA on purpose: the accumulators are exact sums, so the model after the last batch is the
exact PCA of the UNION of all batches (IncrementalPCA's is an approximation that depends on the batch order).  As in the reference
the codec is trained -- usable -- after the first batch.
"""
from typing import Optional

import numpy as np

from .base import BaseCodec

_SHIFT_ROWS = 1024  # rows whose f32 mean is the shift of a fit


def _is_np(x) -> bool:
    return isinstance(x, np.ndarray)


def _finalize(n: int, s: np.ndarray, sum64: np.ndarray, gram64: np.ndarray, n_components: int) -> dict:
    """The host half of a fit, float64 numpy only: ``n`` rows, ``sum64 [D] = sum (x - s)``, ``gram64 [D, D] = sum (x - s)(x - s)^T``
    -> mean, components (rows, sklearn's signs), explained variance and ratio, per-feature variance."""
    s = np.asarray(s, dtype=np.float64)
    sum64 = np.asarray(sum64, dtype=np.float64)
    gram64 = np.asarray(gram64, dtype=np.float64)
    assert n >= 2, 'a PCA needs at least two rows'
    m = sum64 / n
    mean = s + m
    cov = (gram64 - n * np.outer(m, m)) / (n - 1)
    cov = 0.5 * (cov + cov.T)  # (exact for a symmetric gram: eigh reads one triangle)
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(lam)[::-1]
    lam, vec = np.maximum(lam[order], 0.0), vec[:, order]
    comp = vec[:, :n_components].T.copy()
    # sklearn's svd_flip(u_based_decision=False): the entry of largest magnitude of every component is positive
    big = np.argmax(np.abs(comp), axis=1)
    comp *= np.where(comp[np.arange(comp.shape[0]), big] < 0, -1.0, 1.0)[:, None]
    total = float(np.trace(cov))
    return {
        'n': int(n), 'mean': mean, 'components': comp,
        'explained_variance': lam[:n_components].copy(),
        'explained_variance_ratio': lam[:n_components] / total if total > 0 else np.zeros(n_components),
        'var': np.diag(cov) * ((n - 1) / n),
        'covariance': cov,
    }


class ProjectorCodec(BaseCodec):
    """PCA projector: ``dim`` -> ``n_components`` (projector.py:8-58).

    :param n_components: number of components to keep
    :param whiten: scale the projected coordinates to unit variance (components / sqrt(explained variance))
    :param svd_solver: kept for the reference's signature and hash; the fit is always the exact eigen-decomposition
    """

    def __init__(self, dim: int, n_components: int = 128, whiten: Optional[bool] = False, svd_solver: Optional[str] = 'auto'):
        super().__init__(require_train=True)
        self.dim = dim
        self.n_components = n_components
        assert self.dim >= self.n_components, (
            f'the dimension after projector should be less than original dimension, got '
            f'original dimension: {self.dim} and projector dimension: {self.n_components}')
        self.whiten = whiten
        self.svd_solver = svd_solver
        self._model = None  # what `_finalize` returned
        self._dev = {}  # device -> (encode matrix [K, D], decode matrix [D, K], mean [D])
        self._reset()

    def _reset(self):
        self._n = 0
        self._shift = None  # f32 [D], device
        self._sum = None  # f64 [D], device
        self._gram = None  # f64 [D, D], device
        self._ws = None

    def __hash__(self):  # projector.py:49-58
        return hash((self.__class__.__name__, self.dim, self.n_components, self.whiten, self.svd_solver))

    def __getstate__(self):
        st = self.__dict__.copy()
        st['_dev'] = {}
        for key in ('_shift', '_sum', '_gram', '_ws'):  # streaming accumulators do not survive a reload (the model does)
            st[key] = None
        st['_n'] = 0
        return st

    def __setstate__(self, st):
        self.__dict__.update(st)
        self._dev = {}

    # ------------------------------------------------------------------ training
    def _check_input(self, x):
        assert x.ndim == 2
        assert x.shape[1] == self.dim, 'dimension of input data must be equal to "dim"'
        assert x.shape[0] > self.n_components, 'number of input data must be larger than or equal to n_components'

    def _accumulate(self, x):
        import torch

        from ... import ops

        x = ops.to_dev(x, torch.float32)
        if self._shift is None:
            self._shift = x[:_SHIFT_ROWS].mean(dim=0).contiguous()
            self._sum = torch.zeros((self.dim,), dtype=torch.float64, device=x.device)
            self._gram = torch.zeros((self.dim, self.dim), dtype=torch.float64, device=x.device)
            self._ws = ops.ScanWorkspace()
        ops.pca_accumulate(x, self._shift, self._sum, self._gram, self._ws)
        self._n += int(x.shape[0])

    def _finish(self):
        self._model = _finalize(self._n, self._shift.cpu().numpy(), self._sum.cpu().numpy(), self._gram.cpu().numpy(), self.n_components)
        del self._model['covariance']  # (D x D float64: not part of the persisted model)
        self._dev = {}
        self._is_trained = True

    def fit(self, x):
        """projector.py:60-83: the PCA of ``x`` [N, D] (numpy or tensor, float32)."""
        self._check_input(x)
        self._reset()
        self._accumulate(x)
        self._finish()

    def partial_fit(self, x):
        """projector.py:85-107: add a batch.  The shift is fixed by the first batch; after every batch the model is the EXACT PCA of all
        rows seen so far (unlike IncrementalPCA, whose result is approximate and depends on the batch order)."""
        self._check_input(x)
        self._accumulate(x)
        self._finish()

    # ------------------------------------------------------------------ use
    def _matrices(self):
        from ... import ops

        dev = ops.device()
        mats = self._dev.get(dev)
        if mats is None:
            m = self._model
            comp = m['components']
            if self.whiten:
                scale = np.sqrt(m['explained_variance'])[:, None]
                enc, dec = comp / scale, (comp * scale).T
            else:
                enc, dec = comp, comp.T
            mats = self._dev[dev] = (ops.to_dev(np.ascontiguousarray(enc, dtype=np.float32)),
                                     ops.to_dev(np.ascontiguousarray(dec, dtype=np.float32)),
                                     ops.to_dev(np.ascontiguousarray(m['mean'], dtype=np.float32)))
        return mats

    def encode(self, x):
        """projector.py:109-118 (``PCA.transform``): [n, dim] -> [n, n_components]; numpy in -> numpy out, tensor in -> device tensor."""
        import torch

        from ... import ops

        self._check_trained()
        assert x.ndim == 2
        assert x.shape[1] == self.dim, 'dimension of input data must be equal to "dim"'
        enc, _, mean = self._matrices()
        out = ops.affine_rows(ops.to_dev(x, torch.float32), enc, sub=mean)
        return out.cpu().numpy() if _is_np(x) else out

    def decode(self, x):
        """projector.py:120-130 (``PCA.inverse_transform``): [n, n_components] -> [n, dim]."""
        import torch

        from ... import ops

        self._check_trained()
        assert x.ndim == 2
        assert x.shape[1] == self.n_components
        _, dec, mean = self._matrices()
        out = ops.affine_rows(ops.to_dev(x, torch.float32), dec, add=mean)
        return out.cpu().numpy() if _is_np(x) else out

    # ------------------------------------------------------------------ projector.py:132-156
    @property
    def components(self):
        self._check_trained()
        return self._model['components']

    @property
    def explained_variance(self):
        self._check_trained()
        return self._model['explained_variance']

    @property
    def explained_variance_ratio(self):
        self._check_trained()
        return self._model['explained_variance_ratio']

    @property
    def mean(self):
        self._check_trained()
        return self._model['mean']

    @property
    def var(self):
        self._check_trained()
        return self._model['var']

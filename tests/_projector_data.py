"""Planted data with an exact spectrum, shared by the projector tests (CPU and GPU), and the float64 references on it.

``X = sqrt(N - 1) U diag(sqrt(lambda)) Q^T + mu`` rounded to float32: ``U`` [N, D] has orthonormal columns orthogonal to the ones
vector (QR of a column-centred Gaussian), ``Q`` is a random rotation, ``lambda_i = 1 / (1 + i)`` -- so the sample covariance of the
un-rounded data is exactly ``Q diag(lambda) Q^T`` and its mean exactly ``mu``.
"""
import functools

import numpy as np

SHAPES = [(600, 32, 8, 0.0), (4096, 130, 16, 0.0), (4096, 130, 16, 1000.0), (2000, 65, 33, 3.0)]  # (N, D, K, mu)
IDS = ['600x32k8', '4096x130k16', '4096x130k16mu1000', '2000x65k33mu3']
U24 = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def planted(N, D, K, mu):
    """-> dict: x32 (the data), x64 (the same numbers in float64), lam (the planted spectrum), and sklearn's float64 PCA of x64."""
    from sklearn.decomposition import PCA

    rs = np.random.RandomState(N * 131 + D * 7 + K)
    g = rs.randn(N, D)
    U, _ = np.linalg.qr(g - g.mean(axis=0))
    Q, _ = np.linalg.qr(rs.randn(D, D))
    lam = 1.0 / (1.0 + np.arange(D))
    x32 = (np.sqrt(N - 1.0) * (U * np.sqrt(lam)) @ Q.T + mu).astype(np.float32)
    x64 = x32.astype(np.float64)
    pca = PCA(n_components=K, svd_solver='full').fit(x64)
    xc = x64 - x64.mean(axis=0)
    cov64 = xc.T @ xc / (N - 1)
    for a in (x64, cov64, lam):  # (x32 goes through torch.from_numpy, which wants a writable array: nothing writes to it)
        a.setflags(write=False)
    return dict(N=N, D=D, K=K, mu=mu, x32=x32, x64=x64, lam=lam, pca=pca, cov64=cov64)


def signed_cosines(a, b):
    """Row-wise cosine between two sets of components (rows of unit length up to rounding)."""
    return np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def gaps(lam, K):
    """gap_i = distance of lambda_i to the rest of the spectrum, i < K."""
    lam = np.asarray(lam, dtype=np.float64)
    out = np.empty(K)
    for i in range(K):
        left = lam[i - 1] - lam[i] if i > 0 else np.inf
        right = lam[i] - lam[i + 1] if i + 1 < len(lam) else np.inf
        out[i] = min(left, right)
    return out

"""numpy oracle of tl.pca: float64 SVD of the (centred) dense matrix, sklearn 1.7's sign rule
(``svd_flip(u_based_decision=False)``), then the cast.  tests/test_pca_oracle.py pins it to the fixtures
recorded from sklearn; the GPU tests compare tl.pca with it."""
from __future__ import annotations

import glob
import os

import numpy as np
import scipy.sparse as sp

PCA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca")


def default_n_comps(n_obs, n_vars):
    """scanpy's default: 50, or min(n_obs, n_vars) - 1 when that is smaller."""
    return min(50, min(n_obs, n_vars) - 1)


def pca_oracle(X, n_comps, zero_center, dtype=np.float32):
    """(X_pca, components, explained_variance_ratio, explained_variance) as TruncatedSVD(algorithm="arpack")
    (zero_center=False) or PCA(svd_solver="arpack") (zero_center=True) define them."""
    X = X.toarray() if sp.issparse(X) else np.asarray(X)
    X = X.astype(np.float64)
    n = X.shape[0]
    Xc = X - X.mean(axis=0) if zero_center else X
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    U, S, Vt = U[:, :n_comps], S[:n_comps], Vt[:n_comps]
    signs = np.sign(Vt[np.arange(n_comps), np.argmax(np.abs(Vt), axis=1)])
    U, Vt = U * signs, Vt * signs[:, None]
    x_pca = U * S
    if zero_center:
        ev = S**2 / (n - 1)
        ratio = ev / np.var(X, ddof=1, axis=0).sum()
    else:
        ev = np.var(x_pca, axis=0)
        ratio = ev / np.var(X, axis=0).sum()
    return x_pca.astype(dtype), Vt, ratio, ev


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PCA_DIR, "pca_*.npz")))


def load_fixture(name):
    return dict(np.load(os.path.join(PCA_DIR, name + ".npz"), allow_pickle=False))


def ulp_tol(ref):
    """One float32 ulp of every column's largest |value|."""
    m = np.abs(ref).max(axis=0).astype(np.float32)
    return np.spacing(m).astype(np.float64)

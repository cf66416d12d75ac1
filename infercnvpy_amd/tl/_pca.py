"""tl.pca (reference src/infercnvpy/tl/__init__.py:33-75): PCA of X_cnv, the input of neighbours / UMAP / Leiden.

The reference calls ``scanpy.tl.pca(X_cnv, svd_solver="arpack", zero_center=False)``, i.e. sklearn's
``TruncatedSVD(algorithm="arpack")`` (``zero_center=True``: ``PCA(svd_solver="arpack")``).  Here the two passes over
X_cnv run on the GPU and only the W x W eigenproblem on the host:

1. G = X^T X in float64 (icv_gram_f64: float64 MFMA, fixed summation order) and, when centring, the column sums;
2. the top n_comps eigenpairs of G (centred: G - n mu mu^T) with LAPACK's ``evr`` driver, float64;
3. sklearn 1.7's sign rule (``svd_flip(u_based_decision=False)``): each component's largest |entry| (first on ties) is
   positive;
4. X_pca = X V (centred: - mu^T V) on the GPU (icv_project), float64 sums, written as ``dtype``.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

from .. import _engine

_SOLVERS = (None, "arpack", "randomized", "auto", "full", "tsqr", "lobpcg", "covariance_eigh")


def _default_n_comps(n_obs, n_vars):
    return min(50, min(n_obs, n_vars) - 1)


def pca(adata, svd_solver="arpack", zero_center=False, inplace=True, use_rep="cnv", key_added="cnv_pca", *,
        n_comps=None, random_state=0, dtype="float32", return_info=False, **kwargs):
    """Compute the PCA on the result of :func:`infercnvpy_amd.tl.infercnv`.

    Parameters
    ----------
    adata
        annotated data matrix
    svd_solver
        Any value scanpy's ``pp.pca`` accepts.  Every solver gives the exact leading components (the Gram route
        below); the randomized solver's approximation is not emulated.
    zero_center
        False: ``TruncatedSVD`` of X_cnv (the reference's default).  True: ``PCA`` of the column-centred matrix,
        defined as sklearn's ``PCA(svd_solver="arpack")`` on the dense matrix.
    inplace
        If True, store the result in ``adata.obsm[f"X_{key_added}"]``.  Otherwise return it.
    use_rep
        Key under which the result of infercnv is stored in adata (``obsm[f"X_{use_rep}"]``: host CSR, host dense,
        :class:`~infercnvpy_amd.PackedCsr` or a CUDA tensor).
    key_added
        Key under which the result will be stored in adata.obsm if ``inplace=True``.
    n_comps
        Number of components; None: 50, or ``min(n_obs, n_windows) - 1`` when that is smaller (scanpy's default).
    random_state
        Accepted and ignored: the result is exact, nothing is random.
    dtype
        dtype of X_pca (``"float32"``, as scanpy, or ``"float64"``).
    return_info
        Also return ``components`` (n_comps x n_windows), ``explained_variance_ratio`` and ``explained_variance`` with
        sklearn's definitions for ``TruncatedSVD`` (zero_center=False) / ``PCA`` (zero_center=True).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else X_pca, or ``(X_pca, components, explained_variance_ratio,
    explained_variance)`` when ``return_info``.
    """
    if kwargs:
        raise TypeError(f"tl.pca: unsupported keyword argument(s): {', '.join(sorted(kwargs))}")
    if svd_solver not in _SOLVERS:
        raise ValueError(f"tl.pca: unknown svd_solver {svd_solver!r}; one of {_SOLVERS}")
    if f"X_{use_rep}" not in adata.obsm:
        raise KeyError(f"X_{use_rep} is not in adata.obsm. Did you run `tl.infercnv`?")
    dtype = np.dtype(dtype)
    if dtype not in (np.float32, np.float64):
        raise ValueError(f"tl.pca: dtype must be float32 or float64, not {dtype}")
    x = adata.obsm[f"X_{use_rep}"]
    inp = _engine._PcaInput(x)
    n, w = inp.shape
    if n_comps is None:
        n_comps = _default_n_comps(n, w)
    n_comps = int(n_comps)
    if n < 2 or not 1 <= n_comps < min(n, w):
        raise ValueError(f"tl.pca: n_comps={n_comps} must be in [1, min(n_obs, n_vars) = {min(n, w)}) and n_obs >= 2 "
                         f"(X is {n} x {w})")

    g, colsum = _engine.gram(inp, zero_center=True)
    if not np.isfinite(g).all():  # diag(G) = sum of x^2: any NaN / inf of X reaches it
        raise ValueError("Input X contains NaN or infinity.")
    mu = colsum / n
    c = g - n * np.outer(mu, mu) if zero_center else g
    lam, v = scipy.linalg.eigh(c, subset_by_index=[w - n_comps, w - 1], driver="evr")
    lam, v = lam[::-1], np.ascontiguousarray(v[:, ::-1])
    v *= np.sign(v[np.argmax(np.abs(v), axis=0), np.arange(n_comps)])
    shift = mu @ v if zero_center else None
    x_pca = _engine.project(inp, v, shift, np.float64 if return_info else dtype)

    if return_info:
        sq = np.diag(g)
        if zero_center:
            ev = lam / (n - 1)
            ratio = ev / ((sq - n * mu * mu).sum() / (n - 1))
        else:
            ev = np.var(x_pca, axis=0)
            ratio = ev / (sq / n - mu * mu).sum()
        x_pca = x_pca.astype(dtype, copy=False)
    if inplace:
        adata.obsm[f"X_{key_added}"] = x_pca
        return (x_pca, v.T.copy(), ratio, ev) if return_info else None
    return (x_pca, v.T.copy(), ratio, ev) if return_info else x_pca

"""pp.neighbors (reference src/infercnvpy/pp/__init__.py:8-43): the neighbourhood graph of X_cnv_pca.

The reference forwards to ``scanpy.pp.neighbors`` (pynndescent's approximate search above 4 096 cells, umap-learn's
fuzzy simplicial set).  Here both halves run on the GPU and the search is EXACT at every size:

1. the k - 1 nearest other cells of every cell, float64 squared distances of the float32 points, ties to the lower
   index (icv_knn: fp32 MFMA candidate sweep, float64 re-ranking, a certificate per row, an exact kernel for the rows
   that fail it);
2. rho, sigma and the membership strengths of UMAP's ``fuzzy_simplicial_set`` (icv_knn_fuzzy) and the symmetric
   graph ``A + A^T - A o A^T`` as canonical CSR (icv_knn_symmetrize_*).
"""
from __future__ import annotations

import warnings

import numpy as np
import scipy.sparse as sp

from .. import _engine

MAX_NEIGHBORS = 64
MAX_DIMS = 256


def _points(x):
    """The n x d float32 device matrix of a host array or a CUDA tensor (validated)."""
    if type(x).__module__.split(".")[0] == "torch":  # (a host array is validated without touching the GPU)
        import torch

        if x.dim() != 2:
            raise ValueError("pp.neighbors: the representation must be 2-D")
        t = x.to(torch.float32)
        finite = bool(torch.isfinite(t).all().item())
        shape = tuple(t.shape)
    else:
        if sp.issparse(x):
            x = x.toarray()
        a = np.asarray(x)
        if a.ndim != 2:
            raise ValueError("pp.neighbors: the representation must be 2-D")
        with np.errstate(over="ignore"):
            a = np.ascontiguousarray(a, dtype=np.float32)
        finite = bool(np.isfinite(a).all())
        shape, t = a.shape, a
    if not finite:
        raise ValueError("Input X contains NaN or infinity.")
    return t, shape


def neighbors(adata, use_rep="cnv_pca", key_added="cnv_neighbors", inplace=True, *, n_neighbors=15, metric="euclidean",
              method="umap", random_state=0, return_info=False, **kwargs):
    """Compute the neighborhood graph based on the result from :func:`infercnvpy_amd.tl.infercnv`.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        Key under which the PCA of the results of :func:`infercnvpy_amd.tl.infercnv` is stored
        (``obsm[f"X_{use_rep}"]``: host array or CUDA tensor, n x d with d <= 256; converted to float32).  If
        ``"cnv_pca"`` is not present, :func:`infercnvpy_amd.tl.pca` is run with default parameters.
    key_added
        Distances are stored in ``.obsp[key_added + "_distances"]``, connectivities in
        ``.obsp[key_added + "_connectivities"]``, the parameters in ``.uns[key_added]``.
    inplace
        If True, store the neighborhood graph in adata, otherwise return the distance and connectivity matrices.
    n_neighbors
        scanpy's count: the cell itself and its ``n_neighbors - 1`` nearest other cells; 2 .. min(n_obs, 64).
    metric, method
        Only ``"euclidean"`` and ``"umap"``.
    random_state
        Accepted and ignored: the search is exact, nothing is random.
    return_info
        Also return ``knn_indices`` (n x (k - 1) int32, nearest first), ``knn_distances`` (float32), ``rho`` and
        ``sigma`` (float64).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(distances, connectivities)`` (scipy CSR, float32), followed
    by ``knn_indices, knn_distances, rho, sigma`` when ``return_info``.
    """
    if kwargs:
        raise ValueError(f"pp.neighbors: unsupported keyword argument(s): {', '.join(sorted(kwargs))}")
    if metric != "euclidean":
        raise ValueError(f"pp.neighbors: metric {metric!r} is not supported (only 'euclidean')")
    if method != "umap":
        raise ValueError(f"pp.neighbors: method {method!r} is not supported (only 'umap')")
    if f"X_{use_rep}" not in adata.obsm:
        if use_rep != "cnv_pca":
            raise KeyError(f"X_{use_rep} is not in adata.obsm.")
        warnings.warn("X_cnv_pca not found in adata.obsm. Computing PCA with default parameters", stacklevel=2)
        from .. import tl

        tl.pca(adata)
    k = int(n_neighbors)
    if k != n_neighbors:
        raise ValueError(f"pp.neighbors: n_neighbors={n_neighbors!r} is not an integer")
    x, (n, d) = _points(adata.obsm[f"X_{use_rep}"])
    if not 1 <= d <= MAX_DIMS:
        raise ValueError(f"pp.neighbors: the representation has {d} columns; 1 .. {MAX_DIMS} are supported")
    if k < 2 or k > min(n, MAX_NEIGHBORS):
        raise ValueError(f"pp.neighbors: n_neighbors={k} must be in [2, min(n_obs, {MAX_NEIGHBORS}) = "
                         f"{min(n, MAX_NEIGHBORS)}]")

    torch = _engine._torch()
    xd = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x)).cuda().contiguous()
    idx, dist, _n_exact = _engine.knn(xd, k)
    rho, sigma, w = _engine.knn_fuzzy(dist, k)
    c_indptr, c_indices, c_data = _engine.knn_symmetrize(idx, w, k)
    d_indptr, d_indices, d_data = _engine.knn_sorted_rows(idx, dist)
    distances = sp.csr_matrix((d_data.cpu().numpy(), d_indices.cpu().numpy(), d_indptr.cpu().numpy()), shape=(n, n))
    connectivities = sp.csr_matrix((c_data.cpu().numpy(), c_indices.cpu().numpy(), c_indptr.cpu().numpy()),
                                   shape=(n, n))
    info = (idx.cpu().numpy(), dist.cpu().numpy(), rho.cpu().numpy(), sigma.cpu().numpy()) if return_info else ()
    if inplace:
        adata.obsp[key_added + "_distances"] = distances
        adata.obsp[key_added + "_connectivities"] = connectivities
        adata.uns[key_added] = {
            "connectivities_key": key_added + "_connectivities",
            "distances_key": key_added + "_distances",
            "params": {"n_neighbors": k, "method": method, "random_state": random_state, "metric": metric,
                       "use_rep": f"X_{use_rep}"},
        }
        return (distances, connectivities, *info) if return_info else None
    return (distances, connectivities, *info)

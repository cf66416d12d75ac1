"""tl.leiden (reference src/infercnvpy/tl/__init__.py:13-30): cluster the cells by their CNV profiles.

The reference forwards to ``scanpy.tl.leiden`` (leidenalg's randomised, sequential Leiden).  Here a deterministic,
parallel Leiden runs on the GPU by the written contract of DESIGN.md 4.10: integer weights, one float64 gain expression,
a fixed parallel schedule; the labels are a pure function of (graph, resolution, random_state, n_iterations,
use_weights).
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

from .. import _engine


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _graph(adata, neighbors_key, adjacency, obsp):
    if adjacency is not None:
        return adjacency
    if obsp is not None:
        if obsp not in adata.obsp:
            raise KeyError(f"{obsp!r} is not in adata.obsp. Did you run `pp.neighbors`?")
        return adata.obsp[obsp]
    if neighbors_key not in adata.uns:
        raise KeyError(f"{neighbors_key!r} is not in adata.uns. Did you run `pp.neighbors`?")
    key = adata.uns[neighbors_key]["connectivities_key"]
    if key not in adata.obsp:
        raise KeyError(f"{key!r} is not in adata.obsp. Did you run `pp.neighbors`?")
    return adata.obsp[key]


def _host_csr(g, who="tl.leiden"):
    """Canonical CSR arrays (int64, int32, float32 / float64) of a scipy matrix; shape errors before the GPU."""
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise ValueError(f"{who}: the adjacency matrix must be square")
    if g.shape[0] < 1:
        raise ValueError(f"{who}: the adjacency matrix is empty")
    a = sp.csr_matrix(g)
    if a is g:
        a = a.copy()
    a.sum_duplicates()
    a.sort_indices()
    data = a.data if a.data.dtype in (np.float32, np.float64) else a.data.astype(np.float64)
    return a.indptr.astype(np.int64), a.indices.astype(np.int32), np.ascontiguousarray(data)


def leiden(adata, neighbors_key="cnv_neighbors", key_added="cnv_leiden", inplace=True, *, resolution=1.0, random_state=0,
           n_iterations=-1, use_weights=True, directed=None, adjacency=None, obsp=None, return_info=False, **kwargs):
    """Perform Leiden clustering using the CNV neighborhood graph.

    Requires running :func:`infercnvpy_amd.pp.neighbors` first.

    Parameters
    ----------
    adata
        annotated data matrix
    neighbors_key
        Key under which :func:`infercnvpy_amd.pp.neighbors` stored its parameters (``uns[neighbors_key]``).
    key_added
        Key under which the clusters are stored in ``adata.obs``; the parameters go to ``adata.uns[key_added]``.
    inplace
        If True, store the result in adata, otherwise return the ``Categorical`` (the reference returns a copy of the
        AnnData; the duck ``SimpleAnnData`` has no copy, so the arrays are returned as `tl.pca` / `pp.neighbors` do).
    resolution
        gamma of the Reichardt-Bornholdt quality with the configuration null model; a finite float >= 0.
    random_state
        Seed of the counter-based hash behind the vertex priorities (any integer).
    n_iterations
        -1: iterate until an iteration changes nothing (at most 64); N > 0: exactly N iterations.
    use_weights
        False: every stored edge has weight 1.
    directed
        Accepted and ignored (the graph is symmetric: both give the same quality function).
    adjacency, obsp
        The graph itself (scipy sparse matrix of any format / dtype, or a tuple ``(indptr, indices, data)`` of CUDA
        tensors holding a canonical CSR matrix), or the key of one in ``adata.obsp``; they take precedence over
        ``neighbors_key``.
    return_info
        Also return a dict: ``quality`` (Q after every iteration), ``n_iterations`` run, ``levels`` (vertices per level
        of every iteration), ``rounds`` ((local moving, refinement) per level), ``bound_reached``, ``n_communities``.

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else the ``pandas.Categorical`` of the labels ``"0" .. "C-1"``
    (largest community first), followed by the info dict when ``return_info``.
    """
    if kwargs:
        raise ValueError(f"tl.leiden: unsupported keyword argument(s): {', '.join(sorted(kwargs))}")
    try:
        gamma = float(resolution)
    except (TypeError, ValueError):
        raise ValueError(f"tl.leiden: resolution={resolution!r} is not a number") from None
    if not math.isfinite(gamma) or gamma < 0:
        raise ValueError(f"tl.leiden: resolution={resolution!r} must be a finite number >= 0")
    try:
        n_it = int(n_iterations)
        seed = int(random_state)
    except (TypeError, ValueError):
        raise ValueError("tl.leiden: n_iterations and random_state must be integers") from None
    if n_it != n_iterations or (n_it < 1 and n_it != -1):
        raise ValueError(f"tl.leiden: n_iterations={n_iterations!r} must be -1 or a positive integer")
    if seed != random_state:
        raise ValueError(f"tl.leiden: random_state={random_state!r} is not an integer")
    g = _graph(adata, neighbors_key, adjacency, obsp)
    if isinstance(g, (tuple, list)) and len(g) == 3 and all(_is_tensor(t) for t in g):
        dev = g
        n = int(g[0].numel()) - 1
        if n < 1:
            raise ValueError("tl.leiden: the adjacency matrix is empty")
    elif sp.issparse(g):
        dev = None
        host = _host_csr(g)
        n = len(host[0]) - 1
    else:
        raise ValueError("tl.leiden: the graph must be a scipy sparse matrix or (indptr, indices, data) CUDA tensors")
    if adata is not None and hasattr(adata, "n_obs") and adata.n_obs != n:
        raise ValueError(f"tl.leiden: the graph has {n} vertices, adata has {adata.n_obs} cells")
    import pandas as pd

    torch = _engine._torch()
    if dev is None:
        dev = tuple(torch.from_numpy(a).cuda() for a in host)
    indptr, indices, data = dev
    labels, info = _engine.leiden(indptr.to(torch.int64), indices.to(torch.int32), data, gamma, seed, n_it,
                                  bool(use_weights))
    codes = labels.cpu().numpy()
    cats = [str(i) for i in range(info["n_communities"])]
    result = pd.Categorical.from_codes(codes, categories=cats)
    if inplace:
        adata.obs[key_added] = result
        adata.uns[key_added] = {"params": {"resolution": resolution, "random_state": random_state,
                                           "n_iterations": n_iterations}}
        return (result, info) if return_info else None
    return (result, info) if return_info else result

"""tl.leiden (reference src/infercnvpy/tl/__init__.py:13-30): cluster the cells by their CNV profiles.

The reference forwards to ``scanpy.tl.leiden`` (leidenalg's randomised, sequential Leiden).  Here a deterministic,
parallel Leiden runs on the GPU by the written contract of DESIGN.md 4.10: integer weights, one float64 gain expression,
a fixed parallel schedule; the labels are a pure function of (graph, resolution, random_state, n_iterations,
use_weights).
"""
from __future__ import annotations

import math

from .. import _engine
from ._graph import _graph, _host_csr, _is_tensor  # noqa: F401 (their first home: still importable from here)
from ._graph import check_seed, finish, resolve_graph


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
    check_seed("tl.leiden", random_state)
    host, dev, _n = resolve_graph("tl.leiden", adata, neighbors_key, adjacency, obsp)
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
    params = {"resolution": resolution, "random_state": random_state, "n_iterations": n_iterations}
    return finish(adata, "obs", key_added, result, params, info, inplace, return_info)

"""tl.umap (reference src/infercnvpy/tl/__init__.py:78-108): UMAP layout of the CNV neighborhood graph.

The reference forwards to ``scanpy.tl.umap`` (umap-learn's sequential, randomised SGD).  Here the layout is optimised
on the GPU by the written contract of DESIGN.md 4.11: a gather form of umap-learn's ``optimize_layout_euclidean`` in
which every cell is updated from the snapshot of the previous epoch and every row sum is an exact integer sum, so the
coordinates are a pure function of (graph, parameters, random_state, initial positions).  Parity with umap-learn's own
trajectory is not attempted.
"""
from __future__ import annotations

import math
import warnings

import numpy as np
import scipy.sparse as sp

from .. import _engine
from ._graph import (_MASK, _uniform24, check_components, check_seed, finish, init_to_device, resolve_graph,
                     resolve_init)

_TAG_RANDOM, _TAG_NOISE = _MASK, _MASK - 1  # the "epochs" of the counter hash behind the initial positions


def random_init(n, n_components, random_state):
    """init_pos="random": uniform in [-10, 10), a pure function of (n, n_components, random_state)."""
    return (_uniform24(int(random_state), _TAG_RANDOM, n, n_components) * 20.0 - 10.0).astype(np.float32)


def find_ab_params(spread, min_dist):
    """umap-learn's fit of 1 / (1 + a x^(2b)) to the membership curve of (spread, min_dist)."""
    from scipy.optimize import curve_fit

    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


def spectral_init(graph, n_components, random_state):
    """umap-learn's spectral layout of a CONNECTED graph: the eigenvectors 1 .. n_components of the symmetric normalised
    Laplacian (scipy ``eigsh``, start vector of ones), each with its largest-magnitude entry positive, scaled to
    max |y| = 10, plus counter-hash noise of standard deviation 1e-4.  None when the graph has more than one
    connected component or ``eigsh`` does not converge."""
    from scipy.sparse.csgraph import connected_components
    from scipy.sparse.linalg import ArpackError, eigsh

    n = graph.shape[0]
    if n <= n_components + 1 or connected_components(graph, directed=False)[0] != 1:
        return None
    g = graph.astype(np.float64)
    d = 1.0 / np.sqrt(np.asarray(g.sum(axis=0)).ravel())
    D = sp.diags(d)
    L = sp.identity(n, dtype=np.float64) - D @ g @ D
    k = n_components + 1
    try:
        vals, vecs = eigsh(L, k, which="SM", ncv=min(n - 1, max(2 * k + 1, int(math.sqrt(n)))), tol=1e-4, v0=np.ones(n),
                           maxiter=n * 5)
    except (ArpackError, ValueError):
        return None
    y = vecs[:, np.argsort(vals)[1:k]]
    if not np.isfinite(y).all() or not np.abs(y).max() > 0:
        return None
    top = y[np.abs(y).argmax(axis=0), np.arange(n_components)]
    y = y * np.where(top < 0, -1.0, 1.0)
    y = y * (10.0 / np.abs(y).max())
    noise = (_uniform24(int(random_state), _TAG_NOISE, n, n_components) * 2.0 - 1.0) * (math.sqrt(3.0) * 1e-4)
    return (y + noise).astype(np.float32)


def umap(adata, neighbors_key="cnv_neighbors", key_added="cnv_umap", inplace=True, *, min_dist=0.5, spread=1.0,
         n_components=2, maxiter=None, alpha=1.0, gamma=1.0, negative_sample_rate=5, init_pos="spectral", random_state=0,
         a=None, b=None, adjacency=None, obsp=None, return_info=False, **kwargs):
    """Compute the UMAP layout of the CNV neighborhood graph.

    Requires running :func:`infercnvpy_amd.pp.neighbors` first.

    Parameters
    ----------
    adata
        annotated data matrix
    neighbors_key
        Key under which :func:`infercnvpy_amd.pp.neighbors` stored its parameters (``uns[neighbors_key]``).
    key_added
        The layout goes to ``adata.obsm[f"X_{key_added}"]``, the parameters to ``adata.uns[key_added]``.
    inplace
        If True, store the result in adata, otherwise return the array.
    min_dist, spread
        umap-learn's; they determine ``a`` and ``b`` (``scipy.optimize.curve_fit`` on the host) when those are not given.
    n_components
        2 or 3.
    maxiter
        Number of epochs; None: 500 for up to 10 000 cells, else 200.
    alpha, gamma, negative_sample_rate
        Initial learning rate, weight of the negative samples, negative samples per active edge (exactly this many;
        umap-learn's count averages to it).
    init_pos
        ``"spectral"`` (default): umap-learn's spectral layout, computed on the host (see :func:`spectral_init`).  When
        the graph has more than one connected component, or ``eigsh`` does not converge, a warning is issued and
        ``"random"`` is used; umap-learn's per-component layout is not attempted.  ``"random"``: uniform in
        [-10, 10) from the counter hash of ``random_state``.  The name of a key of ``adata.obsm``, or an
        ``n x n_components`` array / CUDA tensor: those positions.
    random_state
        Seed of the counter-based hash behind the negative samples and the initial positions (any integer).
    a, b
        The curve parameters themselves (both or none).
    adjacency, obsp
        The graph itself (scipy sparse matrix, or a tuple ``(indptr, indices, data)`` of CUDA tensors holding a
        canonical CSR matrix), or the key of one in ``adata.obsp``; they take precedence over ``neighbors_key``.
    return_info
        Also return a dict: ``a``, ``b``, ``n_epochs``, ``n_fire`` (stored entries that fire in some epoch),
        ``init_pos`` (what was used) and ``stage_ms`` (validation, epochs).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else the host float32 array ``n x n_components``, followed by the
    info dict when ``return_info``.
    """
    if kwargs:
        raise ValueError(f"tl.umap: unsupported keyword argument(s): {', '.join(sorted(kwargs))}")
    c = check_components("tl.umap", n_components)
    try:
        seed = int(random_state)
        rate = int(negative_sample_rate)
        alpha_f, gamma_f, min_dist_f, spread_f = float(alpha), float(gamma), float(min_dist), float(spread)
    except (TypeError, ValueError):
        raise ValueError("tl.umap: random_state, negative_sample_rate, alpha, gamma, min_dist and spread must be "
                         "numbers") from None
    check_seed("tl.umap", random_state)
    if rate != negative_sample_rate or not 0 <= rate <= 64:
        raise ValueError(f"tl.umap: negative_sample_rate={negative_sample_rate!r} must be an integer in [0, 64]")
    if not (math.isfinite(alpha_f) and alpha_f >= 0 and math.isfinite(gamma_f) and gamma_f >= 0):
        raise ValueError("tl.umap: alpha and gamma must be finite numbers >= 0")
    if (a is None) != (b is None):
        raise ValueError("tl.umap: give both a and b, or neither")
    if a is None and not (math.isfinite(min_dist_f) and math.isfinite(spread_f) and spread_f > 0 and min_dist_f >= 0):
        raise ValueError("tl.umap: min_dist must be >= 0 and spread > 0")
    if a is not None and not (math.isfinite(float(a)) and float(a) > 0 and math.isfinite(float(b)) and float(b) > 0):
        raise ValueError("tl.umap: a and b must be finite numbers > 0")

    host, dev, n = resolve_graph("tl.umap", adata, neighbors_key, adjacency, obsp)
    if maxiter is None:
        n_epochs = 500 if n <= 10_000 else 200
    else:
        n_epochs = int(maxiter)
        if n_epochs != maxiter or n_epochs < 1:
            raise ValueError(f"tl.umap: maxiter={maxiter!r} must be None or a positive integer")

    init = resolve_init("tl.umap", adata, init_pos, ("spectral", "random"), n, c)
    if a is None:
        a, b = find_ab_params(spread_f, min_dist_f)
    a, b = float(a), float(b)

    torch = _engine._torch()
    if dev is None:
        dev = tuple(torch.from_numpy(x).cuda() for x in host)
    indptr, indices, data = (dev[0].to(torch.int64), dev[1].to(torch.int32), dev[2].to(torch.float32))
    used = init if isinstance(init, str) else "given"
    if isinstance(init, str) and init == "spectral":
        if host is None:
            host = tuple(t.cpu().numpy() for t in (indptr, indices, data))
        y0 = spectral_init(sp.csr_matrix((host[2], host[1], host[0]), shape=(n, n)), c, seed)
        if y0 is None:
            warnings.warn("tl.umap: the graph has more than one connected component (or the eigensolver did not "
                          "converge): init_pos='random' is used instead of 'spectral'", UserWarning, stacklevel=2)
            used = init = "random"
        else:
            init = y0
    if isinstance(init, str):
        init = random_init(n, c, seed)
    y = init_to_device("tl.umap", init, indptr.device)
    stage_ms = {}
    _engine.umap_epochs(indptr, indices, data, y, a=a, b=b, gamma=gamma_f, negative_sample_rate=rate,
                        initial_alpha=alpha_f, n_epochs=n_epochs, random_state=seed,
                        stage_ms=stage_ms if return_info else None)
    result = y.cpu().numpy()
    info = None
    if return_info:
        w = data.to(torch.float64)
        n_fire = int(((w > 0) & (w >= w.max() / n_epochs)).sum().item()) if w.numel() else 0
        info = {"a": a, "b": b, "n_epochs": n_epochs, "n_fire": n_fire, "init_pos": used, "stage_ms": stage_ms}
    params = {"a": a, "b": b, "random_state": random_state}
    return finish(adata, "obsm", key_added, result, params, info, inplace, return_info)

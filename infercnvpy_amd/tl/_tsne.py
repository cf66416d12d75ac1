"""tl.tsne (reference src/infercnvpy/tl/__init__.py:111-141): t-SNE layout of the CNV PCA.

The reference forwards to ``scanpy.tl.tsne`` (sklearn's Barnes-Hut ``TSNE``, a randomised and approximated
trajectory).  Here the layout is optimised on the GPU by the written contract of DESIGN.md 4.12: sklearn's sparse
affinities on the exact nearest neighbours, the EXACT repulsion over all ordered pairs (no tree, no angle) and the
update rules of sklearn's ``_gradient_descent``; every sum is an exact integer sum, so the coordinates are a pure
function of (representation, parameters, random_state, initial positions).  Parity with sklearn's own trajectory is not
attempted.
"""
from __future__ import annotations

import math
import time
import warnings

import numpy as np

from .. import _engine
from ..pp._neighbors import MAX_DIMS, _points
from ._graph import (_MASK, _is_tensor, _uniform24, check_components, check_seed, finish, init_to_device,
                     resolve_init)

_TAG_TSNE = _MASK - 2  # the "epoch" of the counter hash behind the random initial positions
MAX_NEIGHBORS = 63
EXAGGERATION_ITERS = 250


def random_init(n, n_components, random_state):
    """init_pos="random": uniform with standard deviation 1e-4, a pure function of (n, n_components, random_state)."""
    u = _uniform24(int(random_state), _TAG_TSNE, n, n_components)
    return ((u * 2.0 - 1.0) * (math.sqrt(3.0) * 1e-4)).astype(np.float32)


def pca_init(x, n_components):
    """init_pos="pca" (sklearn >= 1.2): the first columns of the representation over the float64 standard deviation of
    column 0, times 1e-4, as float32."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if x.shape[1] < n_components:
        raise ValueError(f"tl.tsne: init_pos='pca' needs at least n_components={n_components} columns, the "
                         f"representation has {x.shape[1]}")
    sd = float(np.std(x[:, 0]))
    if not sd > 0.0:
        raise ValueError("tl.tsne: init_pos='pca' needs a first column that is not constant")
    return (x[:, :n_components] / sd * 1e-4).astype(np.float32)


def tsne(adata, use_rep="cnv_pca", key_added="cnv_tsne", inplace=True, *, n_pcs=None, perplexity=30,
         early_exaggeration=12, learning_rate=1000, random_state=0, n_components=2, max_iter=1000, init_pos="pca",
         return_info=False, **kwargs):
    """Compute the t-SNE layout of the result of :func:`infercnvpy_amd.tl.pca`.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        Key of the representation (``obsm[f"X_{use_rep}"]``: host array or CUDA tensor, n x d with d <= 256; converted
        to float32), or the representation itself.  If ``"cnv_pca"`` is not present, :func:`infercnvpy_amd.tl.pca` is
        run with default parameters.  The reference passes ``use_rep="X_cnv_pca"`` to scanpy whatever this argument
        says; here it is honoured.
    key_added
        The layout goes to ``adata.obsm[f"X_{key_added}"]``, the parameters to ``adata.uns[key_added]``.
    inplace
        If True, store the result in adata, otherwise return the array.
    n_pcs
        Use the first ``n_pcs`` columns of the representation (None: all).
    perplexity
        sklearn's; the affinities use the ``min(floor(3 perplexity), 63, n_obs - 1)`` exact nearest neighbours (sklearn
        takes ``3 perplexity`` = 90 at the default; at most 63 are served here) and ``perplexity`` must be below that
        number.
    early_exaggeration, learning_rate
        sklearn's (scanpy's defaults 12 and 1000); the exaggeration and the momentum 0.5 hold for the first 250
        iterations, then 1 and 0.8.
    random_state
        Seed of the counter-based hash behind ``init_pos="random"`` (any integer); nothing else is random.
    n_components
        2 or 3.
    max_iter
        Number of iterations; all of them run (no early stopping: sklearn's ``min_grad_norm`` /
        ``n_iter_without_progress`` would make the count depend on the input).
    init_pos
        ``"pca"`` (default): see :func:`pca_init`.  ``"random"``: see :func:`random_init`.  The name of a key of
        ``adata.obsm``, or an ``n x n_components`` array / CUDA tensor: those positions.
    return_info
        Also return a dict: ``n_neighbors_used``, ``n_iter``, ``init_pos`` (what was used) and ``stage_ms`` (knn,
        affinities, symmetrise, validation, iterations).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else the host float32 array ``n x n_components``, followed by the
    info dict when ``return_info``.
    """
    if kwargs:
        raise ValueError(f"tl.tsne: unsupported keyword argument(s): {', '.join(sorted(kwargs))}")
    c = check_components("tl.tsne", n_components)
    try:
        seed = int(random_state)
        perp, ex, eta = float(perplexity), float(early_exaggeration), float(learning_rate)
    except (TypeError, ValueError):
        raise ValueError("tl.tsne: random_state, perplexity, early_exaggeration and learning_rate must be "
                         "numbers") from None
    check_seed("tl.tsne", random_state)
    if not (math.isfinite(perp) and perp > 0 and math.isfinite(ex) and ex > 0 and math.isfinite(eta) and eta > 0):
        raise ValueError("tl.tsne: perplexity, early_exaggeration and learning_rate must be finite numbers > 0")
    n_iter = int(max_iter)
    if n_iter != max_iter or n_iter < 0:
        raise ValueError(f"tl.tsne: max_iter={max_iter!r} must be a non-negative integer")

    rep_name = use_rep
    if isinstance(use_rep, str):
        if f"X_{use_rep}" not in adata.obsm:
            if use_rep != "cnv_pca":
                raise KeyError(f"X_{use_rep} is not in adata.obsm.")
            warnings.warn("X_cnv_pca not found in adata.obsm. Computing PCA with default parameters", stacklevel=2)
            from . import pca

            pca(adata)
        rep = adata.obsm[f"X_{use_rep}"]
        rep_name = f"X_{use_rep}"
    else:
        rep, rep_name = use_rep, None
    x, (n, d) = _points(rep)
    if n_pcs is not None:
        m = int(n_pcs)
        if m != n_pcs or not 1 <= m <= d:
            raise ValueError(f"tl.tsne: n_pcs={n_pcs!r} must be an integer in [1, {d}]")
        x, d = x[:, :m], m
    if not 1 <= d <= MAX_DIMS:
        raise ValueError(f"tl.tsne: the representation has {d} columns; 1 .. {MAX_DIMS} are supported")
    kk = min(int(math.floor(3.0 * perp)), MAX_NEIGHBORS, n - 1)
    if perp >= kk:
        raise ValueError(f"tl.tsne: perplexity={perplexity!r} must be less than the number of neighbours used, "
                         f"min(floor(3 perplexity), {MAX_NEIGHBORS}, n_obs - 1) = {kk}")

    init = resolve_init("tl.tsne", adata, init_pos, ("pca", "random"), n, c)
    used = init if isinstance(init, str) else "given"
    if isinstance(init, str):
        init = pca_init(x.cpu().numpy() if _is_tensor(x) else x, c) if init == "pca" else random_init(n, c, seed)

    torch = _engine._torch()
    xd = (x if isinstance(x, torch.Tensor) else torch.from_numpy(x)).cuda().contiguous()
    y = init_to_device("tl.tsne", init, xd.device)
    stage_ms = {}

    def timed(name, fn, *args):
        if not return_info:
            return fn(*args)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(*args)
        torch.cuda.synchronize()
        stage_ms[name] = (time.perf_counter() - t0) * 1e3
        return out

    idx, dist, _n_exact = timed("knn_ms", _engine.knn, xd, kk + 1)
    _beta, cond = timed("affinities_ms", _engine.tsne_affinities, dist, perp)
    indptr, indices, data = timed("symmetrise_ms", _engine.tsne_symmetrize, idx, cond)
    u = torch.zeros_like(y)
    gains = torch.ones_like(y)
    _engine.tsne_iterations(indptr, indices, data, y, u, gains, early_exaggeration=ex,
                            exaggeration_iters=EXAGGERATION_ITERS, learning_rate=eta, iter_begin=0, iter_end=n_iter,
                            stage_ms=stage_ms if return_info else None)
    result = y.cpu().numpy()
    info = {"n_neighbors_used": kk, "n_iter": n_iter, "init_pos": used, "stage_ms": stage_ms} if return_info else None
    params = {"perplexity": perplexity, "early_exaggeration": early_exaggeration, "learning_rate": learning_rate,
              "random_state": random_state, "use_rep": rep_name}
    return finish(adata, "obsm", key_added, result, params, info, inplace, return_info)

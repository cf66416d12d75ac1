"""tl.cnv_kmeans: a partition of the cells into a GIVEN number of clones (no counterpart in the reference; R inferCNV's
``k_obs_groups``, the tree cuts of copykat and SCEVAN and the usual tumour / normal split all ask for that number, while
``tl.leiden`` only has a ``resolution``).

Lloyd's k-means on ``X_cnv_pca`` with k-means++ seeding and restarts, by the written contract of DESIGN.md 4.27: every
squared distance is a float64 chain in component order, every sum over cells an int64 sum of values rounded once to a
fixed point, and the seeding draw an integer prefix sum against a counter-based hash.  The result is therefore a pure
function of (representation, k, random_state, n_init, max_iter), equals ``tests/_kmeans_oracle.py`` bit for bit, and its
labels feed every per-clone function and ``tl.cnv_silhouette``, which compares k = 2, 3, 4, ...
"""
from __future__ import annotations

import math
import numbers
import time

import numpy as np

from .. import _engine
from .._lib import ICV_KMEANS_MAX_CLUSTERS as MAX_CLUSTERS, ICV_KMEANS_MAX_SHIFT as MAX_SHIFT
from ._graph import _MASK, _mix_int
from ._silhouette import _representation  # (the same representation under the same cap of 256 components)

_TAG_KMEANS = 0x6B6D65616E73  # "kmeans": the "epoch" of the counter hash behind the seeding draws


def shifts(m, n, n_components):
    """Rule 2: ``(e, f)`` with ``b = frexp(m)[1]``: ``e = min(40, 62 - bit_length(n) - b)`` binary places for a coordinate
    and ``f = min(40, 61 - bit_length(n) - (2b + 2 + bit_length(C - 1)))`` for a squared distance; both 40 when ``m == 0``."""
    if m == 0:
        return MAX_SHIFT, MAX_SHIFT
    b = math.frexp(m)[1]
    nb = int(n).bit_length()
    return (min(MAX_SHIFT, 62 - nb - b), min(MAX_SHIFT, 61 - nb - (2 * b + 2 + int(n_components - 1).bit_length())))


def draws(random_state, n_init, k):
    """Rule 3: per run r the hash values ``z_0 .. z_{k-1}``."""
    out = []
    for r in range(n_init):
        base = _mix_int(((int(random_state) + r) & _MASK) ^ _mix_int(_TAG_KMEANS))
        out.append([_mix_int(base ^ t) for t in range(k)])
    return out


def _whole(who, name, value, lowest):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise TypeError(f"{who}: `{name}` must be an integer, got {value!r}")
    if value < lowest:
        raise ValueError(f"{who}: `{name}` must be at least {lowest}, got {value}")
    return int(value)


def renumber(labels, k):
    """``order`` (``order[j]`` = the raw index of the new cluster j) and the sizes in the new order: the largest cluster
    first, ties in size to the lower raw index, so clusters without cells come last."""
    sizes = np.bincount(labels, minlength=k).astype(np.int64)
    order = np.argsort(-sizes, kind="stable")
    return order, sizes[order]


def cnv_kmeans(adata, n_clusters, *, use_rep="cnv_pca", key_added="cnv_kmeans", random_state=0, n_init=10, max_iter=300,
               init="k-means++", inplace=True, return_info=False):
    """Partition the cells into ``n_clusters`` clones by exact, deterministic k-means of ``X_cnv_pca`` on the GPU.

    ``tl.cnv_kmeans(adata, 2)`` is the tumour / normal split; ``for k in (2, 3, 4): tl.cnv_kmeans(adata, k);
    tl.cnv_silhouette(adata, "cnv_kmeans")`` compares numbers of clones; every per-clone function
    (``cnv_pseudobulk``, ``cnv_segments``, ``cnv_copy_segments``, ``cnv_rank_groups``, ``cnv_correlation(groupby=...)``)
    takes ``groupby="cnv_kmeans"``.

    Parameters
    ----------
    adata
        annotated data matrix
    n_clusters
        k, with 2 <= k <= 256 and k <= n.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x C, 1 <= C <= 256) holds the cells: a host array of any layout, float32 or
        float64 (other dtypes are converted), or a CUDA tensor, which is used where it lies.  Values are used as float64.
    key_added
        ``adata.obs[key_added]`` receives the categorical labels ``"0" .. "k-1"`` (the largest cluster first, ties in size
        to the lower raw index, clusters without cells last, all k categories present),
        ``adata.obs[f"{key_added}_distance"]`` the float64 distance of every cell to its centre (large for an outlier)
        and ``adata.uns[key_added]`` the dict ``{"params", "centers", "sizes", "inertia", "n_iter", "converged",
        "shift", "best_init"}`` (``centers``: k x C float64 in the order of the labels).
    random_state
        The seed of the counter hash behind the k-means++ draws; run r uses ``random_state + r``.
    n_init
        Restarts; the run of lowest inertia wins, ties to the first.  One k-means++ start gets stuck often enough
         for the default of 10.
    max_iter
        Assignments per run at most.  A run that stops there has ``converged=False``; its labels are still the nearest
        centres of the returned ``centers``.
    init
        ``"k-means++"``, or a k x C array of starting centres, which forces one run.  With ``max_iter=1`` a given array
        assigns the cells of another sample to known centres.
    inplace
        If True, store the results in ``adata``, otherwise return ``(codes, centers)`` (int32 n and float64 k x C host
        arrays) and write nothing.
    return_info
        Also return a dict: ``history`` (per run the (integer inertia, n_changed) of every iteration), ``picks`` (per run
        the seeded rows in raw order, None with a given ``init``), ``inertia_q`` (the integer inertia of every run) and
        ``stage_ms`` (host clocks).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``), else ``(codes, centers)``, followed by the info dict when
    ``return_info``.

    With k-means++ the result depends on the order of the rows through the seeding draw, as ``tl.leiden``'s does; with a
    given ``init`` a permutation of the rows permutes the labels and leaves the centres unchanged to the bit.  Values
    too large for exact int64 sums, a non-finite value and fewer distinct points than clusters raise ``ValueError``.
    """
    import pandas as pd
    import torch  # (only to recognise a tensor: the argument checks run without a GPU)

    who = "tl.cnv_kmeans"
    k = _whole(who, "n_clusters", n_clusters, 2)
    n_init = _whole(who, "n_init", n_init, 1)
    max_iter = _whole(who, "max_iter", max_iter, 1)
    random_state = _whole(who, "random_state", random_state, -(1 << 63))
    if k > MAX_CLUSTERS:
        raise ValueError(f"{who}: `n_clusters` must be at most {MAX_CLUSTERS}, got {k}")
    key, x, n, c = _representation(adata, who, use_rep)
    if k > n:
        raise ValueError(f"{who}: `n_clusters` = {k} exceeds the {n} rows of {key}")
    given = None
    if not isinstance(init, str):
        given = np.ascontiguousarray(np.asarray(init), dtype=np.float64)
        if given.shape != (k, c):
            raise ValueError(f"{who}: `init` must be \"k-means++\" or an array of shape {(k, c)}, got {given.shape}")
        if not np.isfinite(given).all():
            raise ValueError(f"{who}: `init` has non-finite values")
    elif init != "k-means++":
        raise ValueError(f"{who}: `init` must be \"k-means++\" or an array of shape {(k, c)}, got {init!r}")

    t0 = time.perf_counter()
    on_device = isinstance(x, torch.Tensor)
    if on_device:
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        dm = _engine.matrix_input(x, who)
        # (one scalar is read back before the launch: the shifts depend on it; a NaN or an infinity shows in it)
        m = float(_engine.states_absmax(dm.dense).item())
    else:
        x = np.asarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        m = float(np.abs(x).max())  # (a NaN stays)
    if not math.isfinite(m):
        raise ValueError(f"{who}: {key} has non-finite values")
    if given is not None:
        m = max(m, float(np.abs(given).max()))
    e, f = shifts(m, n, c)
    if e < 0 or f < 0:
        raise ValueError(f"{who}: values of magnitude {m!r} in {n} rows of {c} components are too large for exact int64 "
                         f"sums: rescale {key}")
    if not on_device:
        dm = _engine.matrix_input(x, who)
    stage_ms = {}
    try:
        res = _engine.kmeans(dm, k, e, f, max_iter, draws=draws(random_state, n_init, k) if given is None else None,
                             init=given, stage_ms=stage_ms)
    except ValueError as err:
        raise ValueError(f"{who}: {key}: {err}") from None
    tt = _engine._torch()
    with tt.cuda.device(dm.device):
        # the one copy of the result to the host: the labels (int32: exact in a float64), D of the labels, the centres
        host = tt.cat([res["labels"].to(tt.float64), res["sqdist"], res["centres"].reshape(-1)]).cpu().numpy()
    raw = host[:n].astype(np.int32)
    order, sizes = renumber(raw, k)
    new_of_raw = np.empty(k, dtype=np.int32)
    new_of_raw[order] = np.arange(k, dtype=np.int32)
    codes = new_of_raw[raw]
    centers = np.ascontiguousarray(host[2 * n:].reshape(k, c)[order])
    best = res["best"]
    stage_ms["kmeans"] = (time.perf_counter() - t0) * 1e3

    if inplace:
        adata.obs[key_added] = pd.Categorical.from_codes(codes, categories=[str(j) for j in range(k)])
        adata.obs[f"{key_added}_distance"] = np.sqrt(host[n:2 * n])
        adata.uns[key_added] = {
            "params": {"n_clusters": k, "use_rep": use_rep, "random_state": random_state, "n_init": len(res["n_iter"]),
                       "max_iter": max_iter, "init": "k-means++" if given is None else "array"},
            "centers": centers, "sizes": sizes, "inertia": float(res["inertia_q"][best]) * 2.0 ** -f,
            "n_iter": res["n_iter"][best], "converged": res["converged"][best], "shift": (e, f), "best_init": best,
        }
    if return_info:
        return codes, centers, {"history": res["history"], "picks": res["picks"], "inertia_q": res["inertia_q"],
                                "stage_ms": stage_ms}
    return None if inplace else (codes, centers)

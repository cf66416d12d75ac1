"""tl.cnv_silhouette: the exact silhouette width of every cell for a partition into clones (no counterpart in the
reference, which leaves the question to the user's own scikit-learn call on ``X_cnv_pca``).

``tl.leiden`` has a ``resolution`` knob and every per-clone function takes ``obs["cnv_leiden"]`` as given; the silhouette
width says how good the partition is: for a cell of clone A, ``a`` is its mean distance to the other cells of A, ``b`` the
smallest mean distance to the cells of another clone and ``s = (b - a) / max(a, b)``.  A cell with ``s < 0`` sits nearer
to another clone (``obs["cnv_silhouette_nearest"]``) than to its own.  All n^2 distances are formed on the GPU and never
stored; by the written contract of DESIGN.md 4.26 every distance is rounded once to a fixed-point int64 and every sum
over pairs is an integer sum, so the result is a pure function of (representation, labels), equals
``tests/_silhouette_oracle.py`` bit for bit and does not depend on the storage or the order of the rows.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine
from .._lib import ICV_SILHOUETTE_MAX_COMPONENTS as MAX_COMPONENTS, ICV_SILHOUETTE_MAX_SHIFT as MAX_SHIFT
from ._groups import group_codes, group_table


def distance_shift(m, largest_group, n_components):
    """Rule 2: ``(e, b + 1 + hc)`` with ``b = frexp(m)[1]`` and ``hc = (bit_length(C - 1) + 1) // 2``: every distance is
    below ``2^(b + 1 + hc)`` and ``e = min(40, 61 - bit_length(L) - (b + 1 + hc))``; ``e = 40`` when ``m == 0``."""
    hc = (int(n_components - 1).bit_length() + 1) // 2
    if m == 0:
        return MAX_SHIFT, 1 + hc
    dist_exp = math.frexp(m)[1] + 1 + hc
    return min(MAX_SHIFT, 61 - int(largest_group).bit_length() - dist_exp), dist_exp


def _representation(adata, who, use_rep):
    """(key, x, n, C) of ``adata.obsm[f"X_{use_rep}"]``, checked without a GPU."""
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{who}: {key} not found in adata.obsm. Did you run `tl.pca`?")
    x = adata.obsm[key]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"{who}: {key} must be 2-D")
    n, c = int(shape[0]), int(shape[1])
    if n < 1 or c < 1:
        raise ValueError(f"{who}: empty matrix of shape {(n, c)}")
    if c > MAX_COMPONENTS:
        raise ValueError(f"{who}: {key} has {c} components; at most {MAX_COMPONENTS} are supported")
    return key, x, n, c


def silhouette_widths(x, codes, n_groups, *, who="tl.cnv_silhouette", key="X", s_budget=None, n_chunks=None,
                      stage_ms=None):
    """Rules 1-5 for the representation ``x`` (host array or CUDA tensor, n x C) and the int64 ``codes`` of the cells
    (-1: no label) in ``n_groups`` groups: a dict of the host arrays ``s``, ``a``, ``b`` (float64 n, NaN without a label)
    and ``nearest`` (int32 n, -1 without a label), ``shift`` and the int64 ``sizes`` of the groups.  ``s_budget`` and
    ``n_chunks`` are passed on to :func:`infercnvpy_amd._engine.silhouette` and change no bit.  The checks that need no
    GPU (the number of groups, host values, the shift) come before any GPU work."""
    import torch  # (only to recognise a tensor: the argument checks run without a GPU)

    n, c = int(x.shape[0]), int(x.shape[1])
    codes = np.asarray(codes, dtype=np.int64)
    if codes.shape[0] != n:
        raise ValueError(f"{who}: {codes.shape[0]} labels for the {n} rows of {key}")
    sizes = np.bincount(codes[codes >= 0], minlength=n_groups).astype(np.int64)
    if np.count_nonzero(sizes) < 2:
        raise ValueError(f"{who}: the silhouette needs at least two groups with cells, got {np.count_nonzero(sizes)}")
    on_device = isinstance(x, torch.Tensor)
    if on_device:
        if x.dtype not in (torch.float32, torch.float64):
            x = x.to(torch.float64)
        dm = _engine.matrix_input(x, who)
        # (one scalar is read back before the launch: the shift depends on it; a NaN or an infinity shows in it)
        m = float(_engine.states_absmax(dm.dense).item())
    else:
        x = np.asarray(x)
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        m = float(np.abs(x).max())  # (a NaN stays)
    if not math.isfinite(m):
        raise ValueError(f"{who}: {key} has non-finite values")
    shift, dist_exp = distance_shift(m, int(sizes.max()), c)
    if shift < 0:
        raise ValueError(f"{who}: values of magnitude {m!r} in groups of up to {int(sizes.max())} cells are too large "
                         f"for an exact int64 sum of distances: rescale {key}")
    rows, group_ptr, _ = group_table(codes, n_groups, sizes=sizes)

    tt = _engine._torch()
    if not on_device:
        dm = _engine.matrix_input(x, who)
    with tt.cuda.device(dm.device):
        s, a, b, nearest, flags = _engine.silhouette(dm, rows, group_ptr, shift, dist_exp, s_budget=s_budget,
                                                     n_chunks=n_chunks, stage_ms=stage_ms)
        # the one copy to the host: the three float64 vectors, the groups (int32: exact) and the flag word
        k = int(rows.shape[0])
        host = tt.cat([s, a, b, nearest.to(tt.float64), flags.to(tt.float64)]).cpu().numpy()
    if int(host[-1]) & 1:
        raise ValueError(f"{who}: {key} has non-finite values")
    out = {}
    for at, name in enumerate(("s", "a", "b")):
        full = np.full(n, np.nan)
        full[rows] = host[at * k:(at + 1) * k]
        out[name] = full
    out["nearest"] = np.full(n, -1, dtype=np.int32)
    out["nearest"][rows] = host[3 * k:4 * k].astype(np.int32)
    out["shift"], out["sizes"] = shift, sizes
    return out


def cnv_silhouette(adata, groupby="cnv_leiden", *, use_rep="cnv_pca", key_added="cnv_silhouette", inplace=True,
                   return_info=False):
    """The silhouette width of every cell for the groups of ``adata.obs[groupby]``, exact and on the GPU.

    ``tl.cnv_silhouette(adata, "cnv_leiden")`` after ``tl.leiden`` tells whether the clones describe the data:
    ``uns["cnv_silhouette"]["mean"]`` compares two resolutions, ``uns["cnv_silhouette"]["groups"]`` shows a clone that
    was split by chance (a low mean) and ``obs["cnv_silhouette"] < 0`` the cells that sit between two clones (doublets,
    normal contamination), with the clone they would otherwise belong to in ``obs["cnv_silhouette_nearest"]``.

    Parameters
    ----------
    adata
        annotated data matrix
    groupby
        A column of ``adata.obs``.  The groups are the categories of a categorical column (an unused one is a group of
        no cells and is skipped), otherwise the distinct values in order of appearance.  A cell with a missing label
        takes no part: it is in no sum and its own width is NaN.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x C, 1 <= C <= 256) holds the cells: a host array of any layout, float32 or
        float64, or a CUDA tensor, which is used where it lies.  Values are used as float64.
    key_added
        ``adata.obs[key_added]`` receives the float64 widths (NaN where unlabelled), ``adata.obs[f"{key_added}_nearest"]``
        the group of smallest mean distance other than the cell's own (categorical over the group labels, missing where
        unlabelled) and ``adata.uns[key_added]`` the dict ``{"groupby", "use_rep", "shift", "mean", "groups"}``:
        ``mean`` is the mean width of the labelled cells and ``groups`` a DataFrame indexed by label with ``n_cells``
        and ``mean`` (NaN for a group of no cells).
    inplace
        If True, store the results in ``adata``, otherwise return ``(s, nearest_codes)`` (float64 and int32 host arrays,
        -1 where unlabelled) and write nothing.
    return_info
        Also return a dict: ``a``, ``b`` (float64 host arrays), ``shift`` and ``stage_ms`` (host clocks; ``widths`` ends
        in the one copy of the result to the host).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``), else ``(s, nearest_codes)``, followed by the info dict when
    ``return_info``.

    With ``d_ij`` the Euclidean distance (float64, the squares added in component order), ``a`` is the mean of ``d_ij``
    over the other cells of the cell's group, ``b`` the smallest mean over the cells of another group and
    ``s = (b - a) / max(a, b)``; ``s = 0`` for the only cell of a group (scikit-learn's convention) and where both
    means are 0.  Every distance is rounded once to a multiple of ``2^-shift`` (``shift = 40`` unless the values or the
    groups are very large), so a mean is within ``2^-(shift + 1)`` of the mean of the float64 distances, and the sums are
    integer sums: the result does not depend on the order of the rows or on how the work is tiled.  The n x n distances
    are never stored; the cost is n^2 C.  Fewer than two groups with cells, a non-finite value and values too large
    for an exact sum raise ``ValueError``.
    """
    import pandas as pd

    who = "tl.cnv_silhouette"
    key, x, n, c = _representation(adata, who, use_rep)
    if groupby not in adata.obs.columns:
        raise KeyError(f"{who}: `{groupby}` not found in `adata.obs`"
                       + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
    codes, labels = group_codes(adata, groupby)

    t0 = time.perf_counter()
    res = silhouette_widths(x, codes, len(labels), who=who, key=key)
    stage_ms = {"widths": (time.perf_counter() - t0) * 1e3}
    s, nearest, sizes = res["s"], res["nearest"], res["sizes"]

    if inplace:
        labelled = codes >= 0
        group_mean = [math.fsum(s[codes == g].tolist()) / int(sizes[g]) if sizes[g] else math.nan
                      for g in range(len(labels))]
        adata.obs[key_added] = s
        adata.obs[f"{key_added}_nearest"] = pd.Categorical.from_codes(nearest, categories=pd.Index(labels))
        adata.uns[key_added] = {
            "groupby": groupby, "use_rep": use_rep, "shift": res["shift"],
            "mean": math.fsum(s[labelled].tolist()) / int(np.count_nonzero(labelled)),
            "groups": pd.DataFrame({"n_cells": sizes, "mean": np.asarray(group_mean, dtype=np.float64)},
                                   index=pd.Index(labels, name=groupby)),
        }
    if return_info:
        return s, nearest, {"a": res["a"], "b": res["b"], "shift": res["shift"], "stage_ms": stage_ms}
    return None if inplace else (s, nearest)

"""tl.cnv_signal and tl.cnv_correlation: the two per-cell scores that tell tumour cells from normal ones and assign cells
to clones (no counterpart in the reference, whose only answer is its R ``copykat`` wrapper).

The CNV signal of a cell is the mean of its squared ``X_cnv`` values; the CNV correlation is Pearson's r between the
cell's profile and a reference profile: the mean of the cells of largest signal (Tirosh 2016, Puram 2017, Neftel 2019),
or the mean profile of every clone.  Malignant cells are high in both, and the profile of largest r is the cell's clone.
Both are formed in one pass over ``X_cnv`` on the GPU by the written contract of DESIGN.md 4.18: float64 sums in window
order with every product rounded before its add, so the result is a pure function of (matrix, profiles), equals
``tests/_correlation_oracle.py`` bit for bit and does not depend on the storage of the matrix.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine
from ._hmm import at_least_one, unit_fraction
from ._pseudobulk import cnv_pseudobulk, mean_profiles, profile_shift


def centre_profiles(p):
    """(c, s2) of rule 1 for ``G x W`` float64 profiles: ``c_g = p_g - fsum(p_g) / W`` and ``s2_g = fsum(c_g c_g)``."""
    g, w = p.shape
    c, s2 = np.empty((g, w), dtype=np.float64), np.empty(g, dtype=np.float64)
    for k in range(g):
        c[k] = p[k] - math.fsum(p[k].tolist()) / w
        s2[k] = math.fsum((c[k] * c[k]).tolist())
    return c, s2


def top_count(who, top_fraction, n):
    """(k, fraction): ``k = max(1, ceil(top_fraction n))`` with the product formed exactly; 0 < top_fraction <= 1."""
    f = unit_fraction(who, "top_fraction", top_fraction)
    return max(1, math.ceil(f * n)), f


def _matrix(adata, who, use_rep):
    """(key, x, n, W) of ``adata.obsm[f"X_{use_rep}"]``, checked as the sibling functions check it."""
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{who}: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    x = adata.obsm[key]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"{who}: {key} must be 2-D")
    n, w = int(shape[0]), int(shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{who}: empty matrix of shape {(n, w)}")
    return key, x, n, w


def _given_profiles(who, profiles, key, w):
    """(G x W float64 host array, names) of the ``profiles`` argument: a container of ``tl.cnv_pseudobulk`` or an array."""
    import torch  # (only to recognise a tensor: the argument checks run without a GPU)

    names = None
    if hasattr(profiles, "obsm") and hasattr(profiles, "obs"):
        if key not in profiles.obsm:
            raise KeyError(f"{who}: {key} not found in profiles.obsm. Did `tl.cnv_pseudobulk` make `profiles`?")
        names = [str(v) for v in profiles.obs.index]
        profiles = profiles.obsm[key]
    if isinstance(profiles, torch.Tensor):
        profiles = profiles.detach().cpu().numpy()  # (small: G x W)
    try:
        p = np.array(profiles, dtype=np.float64, order="C")
    except (TypeError, ValueError):
        raise ValueError(f"{who}: `profiles` must be a G x W array or the container of `tl.cnv_pseudobulk`") from None
    if p.ndim != 2:
        raise ValueError(f"{who}: `profiles` must be 2-D (G x W), got {p.ndim}-D")
    if p.shape[1] != w:
        raise ValueError(f"{who}: `profiles` has {p.shape[1]} windows, {key} has {w}")
    if not np.isfinite(p).all():
        raise ValueError(f"{who}: `profiles` has non-finite values")
    return p, names if names is not None else [str(g) for g in range(p.shape[0])]


def cnv_signal(adata, *, use_rep="cnv", key_added="cnv_signal", inplace=True):
    """The CNV signal of every cell: the mean of its squared CNV values.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  Stored values are used as
        float64, an entry that is not stored is 0.
    key_added
        ``adata.obs[key_added]`` receives the float64 signal.
    inplace
        If True, store the result in ``adata.obs``, otherwise return the float64 host array.

    The squares of a row are summed in window order (DESIGN.md 4.18 rule 2) and divided by W once: the result equals
    ``B / W`` of :func:`cnv_correlation` on the same matrix bit for bit.  On its own the signal separates tumour from
    normal cells only when the alterations are large; use it together with the correlation.  A non-finite value raises
    ``ValueError``.
    """
    who = "tl.cnv_signal"
    key, x, _, _ = _matrix(adata, who, use_rep)
    torch = _engine._torch()
    dm = _engine.matrix_input(x, who)
    with torch.cuda.device(dm.device):
        _, _, signal, _, flags = _engine.profile_corr(dm)
        both = torch.cat([signal, flags.to(torch.float64)]).cpu().numpy()
    if int(both[-1]) & 1:
        raise ValueError(f"{who}: {key} has non-finite values")
    signal = both[:-1].copy()
    if inplace:
        adata.obs[key_added] = signal
        return None
    return signal


def cnv_correlation(adata, profiles=None, *, groupby=None, use_rep="cnv", top_fraction=0.05, min_cells=1,
                    key_added="cnv_correlation", inplace=True, return_info=False):
    """Pearson's r between the CNV profile of every cell and G reference profiles.

    ``tl.cnv_correlation(adata)`` scores every cell against the mean profile of the 5 % of cells of largest CNV signal:
    together with :func:`cnv_signal` it tells tumour cells (high in both) from normal ones.
    ``tl.cnv_correlation(adata, groupby="cnv_leiden")`` scores every cell against the mean profile of every clone, and
    ``tl.cnv_correlation(other, clones)`` assigns the cells of another sample to the clones of
    ``clones = tl.cnv_pseudobulk(adata, "cnv_leiden")``.

    Parameters
    ----------
    adata
        annotated data matrix
    profiles
        The container :func:`cnv_pseudobulk` returns (its ``obsm[f"X_{use_rep}"]`` is used, the profiles are named by
        its ``obs`` index), or a G x W array (a host array or a CUDA tensor; it is copied to the host because it is
        small; the profiles are named ``"0" ... "G-1"``), or None.
    groupby
        With ``profiles=None``: a column of ``adata.obs``; the profiles are the group means of
        ``tl.cnv_pseudobulk(adata, groupby, use_rep=use_rep, min_cells=min_cells)``.  Giving both ``profiles`` and
        ``groupby`` is a ``ValueError``.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) holds the cells: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  Stored values are used as
        float64, an entry that is not stored is 0.
    top_fraction
        in (0, 1]; with ``profiles`` and ``groupby`` both None the single profile, named ``"top"``, is the exact mean
        (the contract of ``tl.cnv_pseudobulk``, its magnitude check included) of the
        ``k = max(1, ceil(top_fraction * n))`` cells of largest signal, ties going to the lower row.  The product is
        formed exactly (``fractions.Fraction``).
    min_cells
        passed on to ``tl.cnv_pseudobulk`` with ``groupby``.
    key_added
        ``adata.obsm[f"X_{key_added}"]`` receives the n x G float64 matrix of r (a numpy array for host input, a CUDA
        tensor for device input), ``adata.obs[key_added]`` the largest r of the row,
        ``adata.obs[f"{key_added}_profile"]`` the name of the lowest profile that has it (categorical over the profile
        names; missing where the whole row is NaN) and ``adata.uns[key_added]`` the dict ``{"profiles": names,
        "source": "profiles" | "groupby" | "top", "use_rep", "groupby", "top_fraction", "top_rows"}``
        (``top_fraction`` is None outside the "top" mode; ``top_rows``, the ascending int64 rows that were averaged,
        is there in the "top" mode only).
    inplace
        If True, store the results in ``adata``, otherwise return ``(r, names)`` and write nothing.
    return_info
        Also return a dict: ``n_profiles``, ``source`` and ``stage_ms`` (host clocks; ``profiles`` ends in the copy of
        the profiles to the host, ``correlation`` in the one copy of the best r and profile of every cell).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``), else ``(r, names)``, followed by the info dict when
    ``return_info``.

    With ``A``, ``B`` and ``D_g`` the float64 sums of ``x``, ``x x`` and ``x c_g[w]`` over the windows of a row in
    ascending order (``c_g`` the profile minus its mean), ``r_g = D_g / sqrt((B - A A / W) s2_g)`` clipped to
    [-1, 1]; it is NaN for a row of no variance (an empty or constant row, W = 1) and for a constant profile.  A
    non-finite stored value or profile raises ``ValueError``, and so does a profile width other than W.

    Two things to keep in mind.  With ``groupby`` and in the "top" mode a cell is part of the mean it is compared
    with: there is no leave-one-out, so r is biased upwards for the cells of a small group (with ``top_fraction`` at
    its default, for the top cells themselves).  And the "top" mode presupposes an event that the tumour cells share:
    the mean of the most aberrant cells is a useful reference only where most of them carry the same alterations.
    """
    import pandas as pd

    who = "tl.cnv_correlation"
    key, x, n, w = _matrix(adata, who, use_rep)
    if profiles is not None and groupby is not None:
        raise ValueError(f"{who}: give `profiles` or `groupby`, not both")
    source = "profiles" if profiles is not None else "groupby" if groupby is not None else "top"
    fraction = top_rows = None
    if source == "top":
        k, fraction = top_count(who, top_fraction, n)
    elif source == "groupby":
        if groupby not in adata.obs.columns:
            raise KeyError(f"{who}: `{groupby}` not found in `adata.obs`"
                           + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
        at_least_one(who, "min_cells", min_cells)
    else:
        p, names = _given_profiles(who, profiles, key, w)

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    t0 = time.perf_counter()
    dm = _engine.matrix_input(x, who)
    with torch.cuda.device(dm.device):
        if source == "groupby":
            p, names = _given_profiles(who, cnv_pseudobulk(adata, groupby, use_rep=use_rep, min_cells=min_cells), key, w)
        elif source == "top":
            _, _, signal, _, flags = _engine.profile_corr(dm)
            order = torch.sort(signal, descending=True, stable=True)[1][:k]  # (stable: ties go to the lower row)
            d_rows = torch.sort(order)[0]
            if int(flags.item()) & 1:
                raise ValueError(f"{who}: {key} has non-finite values")
            mean, _ = mean_profiles(dm, x, d_rows, np.asarray([0, k], dtype=np.int64), profile_shift(k), who, key)
            both = torch.cat([mean.reshape(-1), d_rows.to(torch.float64)]).cpu().numpy()  # (rows < 2^53: exact)
            p, names, top_rows = both[:w].reshape(1, w).copy(), ["top"], both[w:].astype(np.int64)
        t1 = time.perf_counter()
        c, s2 = centre_profiles(p)
        _, _, _, r, flags = _engine.profile_corr(dm, c, s2)
        best_r, best_g = _engine.profile_corr_best(r)
        # the one copy to the host of a device-input call: best r, best profile (an int32: exact) and the flag word
        small = torch.cat([best_r, best_g.to(torch.float64), flags.to(torch.float64)]).cpu().numpy()
        if int(small[-1]) & 1:
            raise ValueError(f"{who}: {key} has non-finite values")
        best_r, best_g = small[:n].copy(), small[n:2 * n].astype(np.int32)
        if not on_device:
            r = r.cpu().numpy()
    info = {"n_profiles": len(names), "source": source,
            "stage_ms": {"profiles": (t1 - t0) * 1e3, "correlation": (time.perf_counter() - t1) * 1e3}}

    if inplace:
        adata.obsm[f"X_{key_added}"] = r
        adata.obs[key_added] = best_r
        adata.obs[f"{key_added}_profile"] = pd.Categorical.from_codes(best_g, categories=pd.Index(names, dtype=object))
        uns = {"profiles": list(names), "source": source, "use_rep": use_rep, "groupby": groupby,
               "top_fraction": float(fraction) if fraction is not None else None}
        if top_rows is not None:
            uns["top_rows"] = top_rows
        adata.uns[key_added] = uns
    if return_info:
        return r, names, info
    return None if inplace else (r, names)

"""tl.cnv_pseudobulk: the exact mean CNV profile of every group of cells (no counterpart in the reference).

R inferCNV runs its HMM on the mean profile of each subcluster, not on single cells: averaging over a clone lowers the
noise of a window by the square root of the clone's size.  Here the profiles of all groups are formed in one pass over
``X_cnv`` on the GPU by the written contract of DESIGN.md 4.17: every stored value is rounded once to a fixed-point
int64, the sums are integer sums, and one division gives the mean.  No floating-point sum is formed, so the result is a
pure function of (matrix, group lists) and equals ``tests/_pseudobulk_oracle.py`` bit for bit, whatever the storage of
the matrix.  The result is a container of its own, one observation per group, on which ``tl.cnv_states`` and its family
run unchanged.
"""
from __future__ import annotations

import time

import numpy as np

from .. import _engine
from .._compat import SimpleAnnData
from ._groups import group_codes, group_table
from ._hmm import at_least_one, chromosome_bounds

MAX_MAGNITUDE = 1024.0  # rule 2: every stored magnitude is below 2^10
MAX_SHIFT = 40


def profile_shift(largest_group):
    """Rule 2: ``min(40, 52 - bit_length(L_max))``, the binary places kept of every value."""
    return min(MAX_SHIFT, 52 - int(largest_group).bit_length())


def group_lists(adata, groupby, n_rows, min_cells, key="X_cnv"):
    """(labels, n_cells, dropped, rows, group_ptr) of the groups of ``adata.obs[groupby]`` with at least ``min_cells``
    cells: the kept labels in group order, their int64 sizes, the labels left out, the int64 row numbers of the kept
    groups' cells sorted by group (ascending inside a group) and the G + 1 positions of the groups in ``rows``.  The
    groups are those of ``tl.cnv_segments``; a missing label belongs to none.  ``ValueError`` when no group is kept."""
    codes, groups = group_codes(adata, groupby)
    if codes.shape[0] != n_rows:
        raise ValueError(f"tl.cnv_pseudobulk: `{groupby}` has {codes.shape[0]} labels for the {n_rows} rows of {key}")
    sizes = np.bincount(codes[codes >= 0], minlength=len(groups)).astype(np.int64)
    kept = np.flatnonzero(sizes >= min_cells)
    dropped = [groups[g] for g in np.flatnonzero(sizes < min_cells)]
    if kept.shape[0] == 0:
        raise ValueError(f"tl.cnv_pseudobulk: no group of `{groupby}` has min_cells={min_cells} cells")
    rows, group_ptr, n_cells = group_table(codes, len(groups), keep=kept, sizes=sizes)
    return groups[kept], n_cells, dropped, rows, group_ptr


def mean_profiles(dm, x, rows, group_ptr, shift, who, key):
    """(mean, fraction), device float64 ``G x W``: rules 3-5 for the listed rows of every group of ``dm``, the device form
    of ``x``, on the current device.  One pair of scalars is read back: ``ValueError`` (prefixed ``who``, naming ``key``)
    for a non-finite value and for a stored magnitude of 1024 or more."""
    total, stored, flags, d_ptr = _engine.group_profiles(dm, rows, group_ptr, shift)
    absmax = _engine.states_absmax(_engine.states_stored_values(dm))
    mean, fraction = _engine.group_profiles_finish(total, stored, d_ptr, shift)
    bits, m = _engine.flag_and_absmax(flags, absmax)
    if bits & 1:
        raise ValueError(f"{who}: {key} has non-finite values")
    if not m < MAX_MAGNITUDE and isinstance(x, _engine.PackedCsr):
        # (the m of a PackedCsr covers the unused tail of its buffers: look at the stored entries alone)
        m = float(_engine.states_absmax(x.data[:x.nnz()]).item())
    if not m < MAX_MAGNITUDE:
        raise ValueError(f"{who}: {key} has a stored value of magnitude {m!r}; the exact sums take "
                         f"magnitudes below {MAX_MAGNITUDE:g}: rescale the matrix or clip the value")
    return mean, fraction


def cnv_pseudobulk(adata, groupby="cnv_leiden", *, use_rep="cnv", min_cells=1, return_info=False):
    """One mean CNV profile per group of cells, as a new container that the HMM functions run on.

    ``clones = tl.cnv_pseudobulk(adata, "cnv_leiden")`` followed by ``tl.cnv_states(clones)``,
    ``tl.cnv_states_fit(clones)``, ``tl.cnv_posteriors(clones)``, ``tl.cnv_states_filter(clones)`` or
    ``tl.cnv_segments(clones)`` calls the alterations of every clone from its mean profile, as R inferCNV's default
    ``analysis_mode = "subclusters"`` does.  ``adata`` is not modified.

    Parameters
    ----------
    adata
        annotated data matrix
    groupby
        A column of ``adata.obs``.  The groups are the categories of a categorical column, otherwise the distinct values
        in order of appearance; cells with a missing label belong to no group and are not read.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) is averaged: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  Stored values are used as float64,
        an entry that is not stored is 0.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    min_cells
        Groups of fewer cells are left out and listed in ``uns["cnv_pseudobulk"]["dropped"]``; that includes the unused
        categories of a categorical column, which have no cells.  ``ValueError`` when no group is left.
    return_info
        Also return a dict: ``n_groups``, ``shift`` and ``stage_ms`` (host clocks; the stage ends in the one copy to the
        host).

    Returns
    -------
    A :class:`infercnvpy_amd.SimpleAnnData` of G observations (the kept groups, in group order) and W variables:

    * ``X`` and ``obsm[f"X_{use_rep}"]``: the same G x W float64 matrix of group means,
    * ``obsm[f"X_{use_rep}_fraction"]``: G x W float64, the share of the group's cells whose stored value at the window
      is not zero,
    * ``uns[use_rep]``: ``{"chr_pos": a copy}``,
    * ``obs``: indexed by ``str(label)``, with the columns ``groupby`` (the label; categorical with the source column's
      categories when that is categorical) and ``n_cells`` (int64),
    * ``uns["cnv_pseudobulk"]``: ``{"groupby", "use_rep", "shift", "dropped"}``.

    Host input gives numpy arrays; device input (``PackedCsr``, CUDA tensor) leaves both matrices on the device as CUDA
    float64 tensors, and one pair of scalars is all that is read back.  With ``e = shift = min(40, 52 - bit_length(L))``
    for the largest kept group of L cells, every value is rounded once to a multiple of ``2^-e`` and all further
    arithmetic is exact up to the one division: a mean is within ``2^-(e+1)`` of the true mean (4.6e-13 up to 4095 cells
    per group, 1.2e-10 at a million).  A non-finite value raises ``ValueError``, and so does a stored magnitude of 1024
    or more.
    """
    import pandas as pd

    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"tl.cnv_pseudobulk: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"tl.cnv_pseudobulk: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    if groupby not in adata.obs.columns:
        raise KeyError(f"tl.cnv_pseudobulk: `{groupby}` not found in `adata.obs`"
                       + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
    x = adata.obsm[key]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"tl.cnv_pseudobulk: {key} must be 2-D")
    n, w = int(shape[0]), int(shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"tl.cnv_pseudobulk: empty matrix of shape {(n, w)}")
    fewest = at_least_one("tl.cnv_pseudobulk", "min_cells", min_cells)
    chr_pos = adata.uns[use_rep]["chr_pos"]
    chromosome_bounds(chr_pos, w)

    labels, n_cells, dropped, rows, group_ptr = group_lists(adata, groupby, n, fewest, key)
    shift = profile_shift(int(n_cells.max()))
    if shift < 0:
        raise ValueError(f"tl.cnv_pseudobulk: a group of {int(n_cells.max())} cells is too large for an exact int64 sum")

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    t0 = time.perf_counter()
    dm = _engine.matrix_input(x, "tl.cnv_pseudobulk")
    with torch.cuda.device(dm.device):
        mean, fraction = mean_profiles(dm, x, rows, group_ptr, shift, "tl.cnv_pseudobulk", key)
        if not on_device:
            mean, fraction = mean.cpu().numpy(), fraction.cpu().numpy()
    stage_ms = {"profiles": (time.perf_counter() - t0) * 1e3}

    source = adata.obs[groupby]
    if isinstance(getattr(source, "dtype", None), pd.CategoricalDtype):
        column = pd.Categorical(labels, categories=source.cat.categories, ordered=bool(source.cat.ordered))
    else:
        column = labels
    obs = pd.DataFrame({groupby: column, "n_cells": n_cells}, index=[str(v) for v in labels])
    out = SimpleAnnData(mean, obs=obs, obsm={key: mean, key + "_fraction": fraction},
                        uns={use_rep: {"chr_pos": dict(chr_pos)},
                             "cnv_pseudobulk": {"groupby": groupby, "use_rep": use_rep, "shift": shift, "dropped": dropped}})
    if return_info:
        return out, {"n_groups": int(labels.shape[0]), "shift": shift, "stage_ms": stage_ms}
    return out

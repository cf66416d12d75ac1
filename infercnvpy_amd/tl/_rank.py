"""tl.cnv_rank_groups: the exact Wilcoxon rank-sum test of every group of cells against the other cells, window by window
(no counterpart in the reference).

After the clustering the question is which regions set a clone apart, and with what significance.  ``X_cnv`` is
thresholded -- most of a column is exactly 0, the rest heavy-tailed -- so the test ranks: per window the cells of the
population are ranked, the doubled mid-ranks of every group are summed, and the normal approximation with the tie
correction gives z, p and the AUC.  The ranking is integer arithmetic on the GPU by the written contract of DESIGN.md
4.20 (doubled mid-ranks, int64 rank sums and tie terms), so the tables are a pure function of (matrix, labels) and equal
``tests/_rank_oracle.py`` on the bytes whatever the storage of the matrix; the few float64 operations that follow run on
the host in numpy, each correctly rounded.
"""
from __future__ import annotations

import time

import numpy as np

from .. import _engine, _lib
from ._groups import group_codes, group_table
from ._hmm import at_least_one, chromosome_bounds
from ._pseudobulk import mean_profiles, profile_shift
from ._segments import _chromosome_names

MAX_CELLS = _lib.ICV_RANK_MAX_CELLS  # rule 2: N^3 fits an int64 below it


def rank_statistics(r2, tie, n_cells, n_pop):
    """(z, p, auc), float64 ``G x W``: rule 3 of DESIGN.md 4.20 from the int64 tables ``r2`` (``G x W``) and ``tie`` (``W``),
    the int64 group sizes and the size N of the population.  Every operation is a correctly rounded float64 one."""
    from scipy.special import erfc

    r2, tie = np.asarray(r2, dtype=np.int64), np.asarray(tie, dtype=np.int64)
    n_total = int(n_pop)
    n1 = np.asarray(n_cells, dtype=np.int64)[:, None]
    n2 = n_total - n1
    u2 = r2 - n1 * (n1 + 1)
    d2 = u2 - n1 * n2
    k = (np.int64(n_total ** 3 - n_total) - tie).astype(np.float64)[None, :]
    degenerate = (k == 0.0) | (n2 == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        var = ((n1 * n2).astype(np.float64) * k) / float(12 * n_total * (n_total - 1))
        z = (d2.astype(np.float64) / 2.0) / np.sqrt(var)
        auc = u2.astype(np.float64) / (2 * n1 * n2).astype(np.float64)
    z = np.where(degenerate, 0.0, z)
    p = np.where(degenerate, 1.0, erfc(np.abs(z) / np.sqrt(2.0)))
    auc = np.where(np.broadcast_to(n2 == 0, auc.shape), 0.5, auc)
    return z, p, auc


def benjamini_hochberg(p):
    """Rule 4: the adjusted p of every row of ``p`` (``G x W``) over its W windows."""
    p = np.asarray(p, dtype=np.float64)
    w = p.shape[1]
    order = np.argsort(p, axis=1, kind="stable")
    q = np.take_along_axis(p, order, axis=1) * float(w) / np.arange(1, w + 1, dtype=np.float64)[None, :]
    q = np.minimum(np.minimum.accumulate(q[:, ::-1], axis=1)[:, ::-1], 1.0)
    out = np.empty_like(p)
    np.put_along_axis(out, order, q, axis=1)
    return out


def population_codes(codes, kept, n_groups):
    """int32 per cell: -1 for a missing label, 0 .. len(kept) - 1 for the cells of the tested groups (``kept``: their
    ascending numbers among the ``n_groups`` groups) and len(kept) for the cells of the others, who are ranked too."""
    new_code = np.full(n_groups + 1, len(kept), dtype=np.int32)
    new_code[kept] = np.arange(len(kept), dtype=np.int32)
    new_code[n_groups] = -1  # (the slot the code -1 indexes)
    return new_code[codes]


def regions_table(z, pvals_adj, auc, labels, n_cells, chr_pos, bounds, alpha, min_windows):
    """The ``"regions"`` DataFrame: the maximal runs, inside one chromosome, of windows with ``pvals_adj < alpha`` and one
    sign of z, found by ``_engine.segments_tables`` on the int8 sign matrix."""
    import pandas as pd

    torch = _engine._torch()
    sign = np.where(pvals_adj < alpha, np.sign(z), 0.0).astype(np.int8)
    _, _, row, start, end, state, _ = _engine.segments_tables(torch.from_numpy(np.ascontiguousarray(sign)).cuda(), bounds)
    row, start, end, state = (v.cpu().numpy() for v in (row, start, end, state))
    n_windows = (end - start).astype(np.int32)
    keep = n_windows >= min_windows
    row, start, end, state, n_windows = row[keep], start[keep], end[keep], state[keep], n_windows[keep]
    score, worst, mean_auc = (np.empty(row.shape[0], dtype=np.float64) for _ in range(3))
    for i, (g, a, b) in enumerate(zip(row, start, end)):
        score[i] = z[g, a + int(np.argmax(np.abs(z[g, a:b])))]  # (argmax: the lowest window of a tie)
        worst[i] = pvals_adj[g, a:b].max()
        mean_auc[i] = auc[g, a:b].mean()
    return pd.DataFrame({"group": labels[row], "chromosome": _chromosome_names(chr_pos, start), "start": start, "end": end,
                         "direction": state, "n_windows": n_windows, "n_cells": n_cells[row], "score": score,
                         "pvals_adj_max": worst, "auc": mean_auc})


def cnv_rank_groups(adata, groupby="cnv_leiden", *, use_rep="cnv", min_cells=2, alpha=0.05, min_windows=1,
                    key_added="cnv_rank_groups", inplace=True, return_info=False):
    """Which windows set each group of cells apart from the other cells: the Wilcoxon rank-sum test per group and window.

    The counterpart of ``scanpy.tl.rank_genes_groups(method="wilcoxon")`` for ``X_cnv``.  The population is every cell
    with a label, N of them; every group of at least ``min_cells`` cells is tested, in every window, against the rest of
    the population (the cells of smaller groups stay in the rest).  Tie-corrected, no continuity correction.

    Parameters
    ----------
    adata
        annotated data matrix
    groupby
        A column of ``adata.obs``, read as ``tl.cnv_pseudobulk`` reads it; cells with a missing label are not ranked.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  An entry that is not stored is 0,
        and so are a stored ``0.0`` and ``-0.0``.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every
        chromosome.
    min_cells
        Groups of fewer cells are not tested and are listed under ``"dropped"``.  ``ValueError`` when no group is left.
    alpha
        A window is significant where ``pvals_adj < alpha``; in (0, 1].
    min_windows
        Regions of fewer windows are left out of ``"regions"``.
    key_added
        ``adata.uns[key_added]`` receives the result when ``inplace``.
    return_info
        Also return a dict: ``n_groups``, ``n_entries`` (the ranked values that are not 0), ``n_tiles`` (the window tiles
        the ranking ran in) and ``stage_ms`` (host clocks of ``tables``, ``means`` and ``finish``, and the device-event
        times of the ranking's stages ``count``, ``scatter``, ``sort``, ``rank_sums`` and ``finish_kernel``).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``), else the result dict, followed by the info dict when
    ``return_info``.  The result holds host numpy arrays for every kind of input:

    * ``"groups"`` the G tested labels, ``"n_cells"`` their int64 sizes, ``"dropped"`` the labels left out,
    * ``"scores"`` (z), ``"pvals"``, ``"pvals_adj"`` (Benjamini-Hochberg over the W windows of a group) and ``"auc"``:
      G x W float64 each; z > 0 and auc > 0.5 where the group's values are the larger ones,
    * ``"mean"``: G x W float64, the exact group means of ``tl.cnv_pseudobulk``,
    * ``"chr_pos"`` a copy, ``"params"``,
    * ``"regions"``: a DataFrame of the maximal runs, inside one chromosome, of significant windows with one sign of z:
      ``group``, ``chromosome``, ``start``, ``end`` (window numbers, ``end`` exclusive), ``direction`` (int8 +1 / -1),
      ``n_windows``, ``n_cells``, ``score`` (the z of largest magnitude, the lowest window at a tie),
      ``pvals_adj_max`` and ``auc`` (the mean over the run), ordered by (group, start).

    A non-finite value raises ``ValueError``, so does a stored magnitude of 1024 or more (the exact means) and a population
    of 2^21 cells or more.
    """
    who = "tl.cnv_rank_groups"
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{who}: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"{who}: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    if groupby not in adata.obs.columns:
        raise KeyError(f"{who}: `{groupby}` not found in `adata.obs`"
                       + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
    x = adata.obsm[key]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"{who}: {key} must be 2-D")
    n, w = int(shape[0]), int(shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{who}: empty matrix of shape {(n, w)}")
    fewest = at_least_one(who, "min_cells", min_cells)
    try:
        level = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: alpha={alpha!r} must be a number in (0, 1]") from None
    if isinstance(alpha, bool) or not 0.0 < level <= 1.0:
        raise ValueError(f"{who}: alpha={alpha!r} must be a number in (0, 1]")
    shortest = at_least_one(who, "min_windows", min_windows)
    chr_pos = adata.uns[use_rep]["chr_pos"]
    bounds = chromosome_bounds(chr_pos, w, who)

    codes, groups = group_codes(adata, groupby)
    if codes.shape[0] != n:
        raise ValueError(f"{who}: `{groupby}` has {codes.shape[0]} labels for the {n} rows of {key}")
    sizes = np.bincount(codes[codes >= 0], minlength=len(groups)).astype(np.int64)
    kept = np.flatnonzero(sizes >= fewest)
    dropped = [groups[g] for g in np.flatnonzero(sizes < fewest)]
    if kept.shape[0] == 0:
        raise ValueError(f"{who}: no group of `{groupby}` has min_cells={fewest} cells")
    n_pop = int(sizes.sum())
    if n_pop >= MAX_CELLS:
        raise ValueError(f"{who}: {n_pop} cells have a label; at most {MAX_CELLS - 1} are ranked against each other "
                         f"(N^3 in an int64)")
    rows, group_ptr, n_cells = group_table(codes, len(groups), keep=kept, sizes=sizes)
    labels = groups[kept]
    code = population_codes(codes, kept, len(groups))

    torch = _engine._torch()
    stage_ms, info = {}, {}
    t0 = time.perf_counter()
    dm = _engine.matrix_input(x, who)
    with torch.cuda.device(dm.device):
        device_ms = {} if return_info else None
        r2, tie, bits = _engine.rank_tables(dm, code, n_cells, stage_ms=device_ms, info=info)
        if bits & 1:
            raise ValueError(f"{who}: {key} has non-finite values")
        r2, tie = r2.cpu().numpy(), tie.cpu().numpy()
        t1 = time.perf_counter()
        mean, _ = mean_profiles(dm, x, rows, group_ptr, profile_shift(int(n_cells.max())), who, key)
        mean = mean.cpu().numpy()
        t2 = time.perf_counter()
        z, p, auc = rank_statistics(r2, tie, n_cells, n_pop)
        p_adj = benjamini_hochberg(p)
        regions = regions_table(z, p_adj, auc, labels, n_cells, chr_pos, bounds, level, shortest)
    stage_ms.update(tables=(t1 - t0) * 1e3, means=(t2 - t1) * 1e3, finish=(time.perf_counter() - t2) * 1e3)
    if device_ms is not None:
        stage_ms.update({("finish_kernel" if k == "finish" else k): v for k, v in device_ms.items()})

    out = {"groups": labels, "n_cells": n_cells, "scores": z, "pvals": p, "pvals_adj": p_adj, "auc": auc, "mean": mean,
           "chr_pos": dict(chr_pos), "dropped": dropped, "regions": regions,
           "params": {"groupby": groupby, "use_rep": use_rep, "min_cells": fewest, "alpha": level, "min_windows": shortest,
                      "n_population": n_pop}}
    if inplace:
        adata.uns[key_added] = out
    if return_info:
        return out, {"n_groups": int(labels.shape[0]), "n_entries": info["n_entries"], "n_tiles": info["n_tiles"],
                     "stage_ms": stage_ms}
    return None if inplace else out

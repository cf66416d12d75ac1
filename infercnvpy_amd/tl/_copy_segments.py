"""tl.cnv_copy_segments: the level-aware segment tables of the calls of ``tl.cnv_copy_states`` (no counterpart in the
reference).

R inferCNV's multi-level HMM ends in tables of regions, each with its copy-number state and a probability.
``tl.cnv_segments`` tabulates -1 / 0 / +1 only: on the sign plane a step from one to two copies gained is one segment.
Here a run is a maximal stretch of ONE level inside one chromosome (the run of ``tl.cnv_copy_states_filter``), every
per-cell segment carries the mean P(neutral) that the filter would judge it by, and with ``groupby`` the cells of every
group vote per window and per level.  Integer arithmetic throughout: every table equals
``tests/_copy_segments_oracle.py`` byte for byte.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine, _lib
from ._groups import group_codes, group_table
from ._hmm import at_least_one, call_matrix, chromosome_bounds, unit_fraction
from ._segments import _chromosome_names

_WHO = "tl.cnv_copy_segments"
_TWO40 = 1099511627776.0


def _level_range(adata, level_range, states_key):
    """(lo, hi): ``level_range``, else what the model of ``adata.uns[states_key]["params"]`` spans, else (-7, 7)."""
    top = _lib.ICV_LEVEL_MAX
    if level_range is None:
        stored = adata.uns[states_key] if states_key is not None and states_key in adata.uns else None
        if isinstance(stored, dict) and "params" in stored and "levels" in stored["params"] and "neutral" in stored["params"]:
            z = int(stored["params"]["neutral"])
            level_range = (-z, len(stored["params"]["levels"]) - 1 - z)
        else:
            level_range = (-top, top)
    try:
        lo, hi = level_range
        ok = not isinstance(lo, bool) and not isinstance(hi, bool) and int(lo) == lo and int(hi) == hi
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{_WHO}: level_range={level_range!r} must be a pair of integers (lo, hi)")
    lo, hi = int(lo), int(hi)
    if not -top <= lo <= 0 <= hi <= top:
        raise ValueError(f"{_WHO}: level_range=({lo}, {hi}) must satisfy -{top} <= lo <= 0 <= hi <= {top}")
    return lo, hi


def cnv_copy_segments(adata, groupby=None, *, use_rep="cnv_copy_states", posterior_key="cnv_copy_posterior",
                      states_key="cnv_copy_states", level_range=None, cnv_key="cnv", key_added="cnv_copy_segments",
                      min_fraction=0.5, min_windows=1, inplace=True, return_info=False):
    """Tables of the altered segments of every cell (``groupby=None``) or of every group of cells, by copy-number level.

    A segment is a maximal run of windows with one level other than 0 inside one chromosome: ``+1 +1 +2 +2`` is two
    segments, as in :func:`infercnvpy_amd.tl.cnv_copy_states_filter`.  Requires running
    :func:`infercnvpy_amd.tl.cnv_copy_states` first, and :func:`infercnvpy_amd.tl.cnv_copy_posteriors` for ``p_neutral``.

    Parameters
    ----------
    adata
        annotated data matrix
    groupby
        None: one row per segment of every cell.  A column of ``adata.obs`` (``"cnv_leiden"``): the cells of every group
        vote per window and level, and the segments are those of the group's consensus levels.  Groups are formed as in
        :func:`infercnvpy_amd.tl.cnv_segments`: the categories of a categorical column (an unused category is a group of
        no cells), otherwise the distinct values in order of appearance; cells with a missing label belong to no group.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` is the int8 n x W matrix of levels (0 neutral, ``-d`` / ``+d`` a loss / gain of
        distance d): a host numpy array (uploaded once) or a CUDA int8 tensor (read where it lies).
    posterior_key
        Per cell only.  If ``adata.obsm[f"X_{posterior_key}_neutral"]`` exists (float64 n x W, a host array or a CUDA
        tensor) the table gets ``p_neutral``; None switches that off, and a missing plane gives no column.
    states_key, level_range
        The levels must lie in ``[lo, hi]`` with ``-7 <= lo <= 0 <= hi <= 7``: ``level_range`` if it is given, else
        ``(-z, K - 1 - z)`` for the K levels and the neutral index z of ``adata.uns[states_key]["params"]`` (what
        ``tl.cnv_copy_states`` leaves), else (-7, 7).  With ``groupby`` one plane of counts is kept per level of the range.
    cnv_key
        ``adata.uns[cnv_key]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        ``adata.uns[key_added]`` receives a dict: ``"segments"`` (the DataFrame), ``"params"`` (with the resolved
        ``"level_range"``) and, with ``groupby``, ``"groups"`` (the labels), ``"n_cells"`` (int64 per group),
        ``"consensus"`` (int8 G x W levels), ``"levels"`` (the list lo .. hi), ``"counts"`` (int32 G x P x W: the cells of
        the group at level ``levels[p]``, the neutral plane included), ``"loss"`` and ``"gain"`` (int32 G x W: the cells at
        any level below / above 0).
    min_fraction
        in (0, 1].  The sign of a group's consensus at a window is that of ``tl.cnv_segments``: + (-) when at least
        ``max(1, ceil(min_fraction * n_cells))`` of its cells have a gain (loss) of any level and more cells than have
        the opposite sign; the product is formed exactly.  The level is the most frequent one of that sign among the
        group's cells, the one nearest to 0 on a tie.
    min_windows
        Segments of fewer windows are dropped from the table (after it was formed: a mask on the host).
    inplace
        If True, store the result in ``adata.uns``, otherwise return it.
    return_info
        Also return a dict: ``n_segments`` (before ``min_windows``), ``n_groups`` and ``stage_ms`` (host clocks around
        each device stage; each stage ends in a copy to the host).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else the DataFrame, with ``groupby`` the tuple
    ``(DataFrame, consensus, loss, gain, counts)`` of host arrays, followed by the info dict when ``return_info``.

    Per cell the columns are ``cell`` (int64 row number), ``chromosome``, ``start``, ``end`` (int32 window numbers,
    ``end`` exclusive), ``level`` (int8), ``n_windows`` (int32) and ``p_neutral`` (float64), ordered by (cell, start).
    With ``q = rint(P 2^40)`` per window, ``p_neutral = float(sum(q)) / (float(n_windows) 2^40)``: the very mean that
    ``tl.cnv_copy_states_filter`` compares with ``max_p_normal``, so ``p_neutral > t`` selects exactly the runs it would
    remove at ``max_p_normal=t``.  Only the posteriors inside runs are read.

    Per group the columns are ``group``, ``chromosome``, ``start``, ``end``, ``level``, ``n_windows``, ``n_cells`` (int64,
    the group's size), ``cells_min`` (int32) and ``support`` (float64): the fewest, and the mean share, over the segment's
    windows of the group's cells that carry the segment's *sign*; ``level_cells_min`` and ``level_support``: the same for
    the cells that carry exactly the segment's *level*.  There is no ``p_neutral`` per group.  The probability of a
    clone's segment comes from the clone's own profile: ``clones = tl.cnv_pseudobulk(adata, groupby, ...)``, then
    ``tl.cnv_copy_states`` and ``tl.cnv_copy_posteriors`` on ``clones``, then ``tl.cnv_copy_segments(clones)``.

    With ``use_rep="cnv_states"`` and ``posterior_key="cnv_posterior"`` (the three-state pair) the tables are those of
    ``tl.cnv_segments`` with ``level`` for ``state``, plus ``p_neutral``.

    A level outside ``[lo, hi]`` raises ``ValueError`` (one flag read back from the device); so does a posterior inside
    a run that is not a number in [0, 1], and a plane whose shape is not that of the levels or that is not float64.
    """
    import pandas as pd

    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{_WHO}: {key} not found in adata.obsm. Did you run `tl.cnv_copy_states`?")
    x, _, _, w = call_matrix(adata, _WHO, key, cnv_key, "`tl.cnv_copy_states`? (it reads what `tl.infercnv` leaves there)")
    chr_pos = adata.uns[cnv_key]["chr_pos"]
    bounds = chromosome_bounds(chr_pos, w, _WHO)
    fraction = unit_fraction(_WHO, "min_fraction", min_fraction)
    shortest = at_least_one(_WHO, "min_windows", min_windows)
    lo, hi = _level_range(adata, level_range, states_key)
    params = {"groupby": groupby, "use_rep": use_rep, "posterior_key": posterior_key, "level_range": (lo, hi),
              "min_fraction": float(fraction), "min_windows": shortest}
    post = None
    if groupby is not None:
        if groupby not in adata.obs.columns:
            raise ValueError(f"{_WHO}: `{groupby}` not found in `adata.obs`"
                             + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
        codes, groups = group_codes(adata, groupby)
        n_groups = len(groups)
        rows, group_ptr, n_cells = group_table(codes, n_groups)
        need = np.asarray([max(1, math.ceil(fraction * int(c))) for c in n_cells], dtype=np.int32)
    elif posterior_key is not None and f"X_{posterior_key}_neutral" in adata.obsm:
        pkey = f"X_{posterior_key}_neutral"
        post = adata.obsm[pkey]
        if tuple(getattr(post, "shape", ())) != tuple(x.shape):
            raise ValueError(f"{_WHO}: {pkey} has shape {tuple(getattr(post, 'shape', ()))}, {key} has {tuple(x.shape)}")
        if str(getattr(post, "dtype", None)) not in ("float64", "torch.float64"):
            raise ValueError(f"{_WHO}: {pkey} must be float64, not {getattr(post, 'dtype', type(post).__name__)}")
    outside = f"{_WHO}: {key} has levels outside [{lo}, {hi}]"

    torch = _engine._torch()
    stage_ms = {}
    t0 = time.perf_counter()
    states = _engine.dense_input(x)
    with torch.cuda.device(states.device):
        if groupby is None:
            _, _, d_row, d_start, d_end, level, bad = _engine.level_segments_tables(states, bounds, lo, hi)
            if int(bad.item()):
                raise ValueError(outside)
            row, start, end, level = (v.cpu().numpy() for v in (d_row, d_start, d_end, level))
            t1 = time.perf_counter()
            stage_ms["segments"] = (t1 - t0) * 1e3
            psum = None
            if post is not None:
                psum, bad_p = _engine.segments_psum(_engine.dense_input(post), d_row, d_start, d_end)
                psum = psum.cpu().numpy()
                if int(bad_p.item()):
                    raise ValueError(f"{_WHO}: {pkey} has a posterior inside a run that is not a number in [0, 1]")
                stage_ms["psum"] = (time.perf_counter() - t1) * 1e3
        else:
            counts, bad = _engine.level_votes(states, rows, group_ptr, lo, hi)
            loss, gain, consensus = _engine.level_consensus(counts, need, lo, hi)
            if int(bad.item()):
                raise ValueError(outside)
            t1 = time.perf_counter()
            stage_ms["votes"] = (t1 - t0) * 1e3
            if n_groups:
                _, _, row, start, end, level, _ = _engine.level_segments_tables(consensus, bounds, lo, hi)
                support = _engine.level_segments_support(row, start, end, level, counts, loss, gain, lo, hi)
                row, start, end, level = (v.cpu().numpy() for v in (row, start, end, level))
                cells_min, cells_sum, level_min, level_sum = (v.cpu().numpy() for v in support)
            else:
                row, cells_sum, level_sum = (np.zeros(0, dtype=np.int64) for _ in range(3))
                start, end, cells_min, level_min = (np.zeros(0, dtype=np.int32) for _ in range(4))
                level = np.zeros(0, dtype=np.int8)
            consensus, loss, gain, counts = (v.cpu().numpy() for v in (consensus, loss, gain, counts))
            stage_ms["segments"] = (time.perf_counter() - t1) * 1e3

    n_segments = int(row.shape[0])
    n_windows = (end - start).astype(np.int32)
    keep = n_windows >= shortest
    columns = {"cell" if groupby is None else "group": row if groupby is None else groups[row],
               "chromosome": _chromosome_names(chr_pos, start), "start": start, "end": end, "level": level,
               "n_windows": n_windows}
    if groupby is None:
        if psum is not None:
            columns["p_neutral"] = psum.astype(np.float64) / (n_windows.astype(np.float64) * _TWO40)
    else:
        size = n_cells[row]
        cells = (n_windows.astype(np.int64) * size).astype(np.float64)
        columns["n_cells"] = size
        columns["cells_min"] = cells_min
        columns["support"] = cells_sum.astype(np.float64) / cells
        columns["level_cells_min"] = level_min
        columns["level_support"] = level_sum.astype(np.float64) / cells
    table = pd.DataFrame({k: v[keep] for k, v in columns.items()})
    info = {"n_segments": n_segments, "n_groups": n_groups if groupby is not None else 0, "stage_ms": stage_ms}

    result = (table,) if groupby is None else (table, consensus, loss, gain, counts)
    if inplace:
        out = {"segments": table, "params": params}
        if groupby is not None:
            out.update(groups=groups, n_cells=n_cells, consensus=consensus, levels=list(range(lo, hi + 1)), counts=counts,
                       loss=loss, gain=gain)
        adata.uns[key_added] = out
    if return_info:
        return (*result, info)
    if inplace:
        return None
    return table if groupby is None else result

"""tl.cnv_segments: the altered segments of every cell, or of every group of cells (no counterpart in the reference).

``tl.cnv_states`` leaves an n x W int8 matrix of loss / neutral / gain calls; R inferCNV's HMM output ends in tables of
segments.  Here the runs of every row are compacted on the GPU (count, scan, fill), and with ``groupby`` the calls of
every group's cells are counted per window, a consensus row per group is formed and its runs are the group's segments
(DESIGN.md 4.14).  Integer arithmetic throughout: every table equals ``tests/_segments_oracle.py`` byte for byte.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine
from ._groups import group_codes, group_table
from ._hmm import at_least_one, call_matrix, chromosome_bounds, unit_fraction


def _chromosome_names(chr_pos, starts):
    """The name of the chromosome that holds each window of ``starts``."""
    names = np.asarray([k for k, _ in sorted(chr_pos.items(), key=lambda kv: int(kv[1]))], dtype=object)
    first = np.asarray(sorted(int(v) for v in chr_pos.values()), dtype=np.int64)
    return names[np.searchsorted(first, np.asarray(starts, dtype=np.int64), side="right") - 1]


def cnv_segments(adata, groupby=None, *, use_rep="cnv_states", cnv_key="cnv", key_added="cnv_segments", min_fraction=0.5,
                 min_windows=1, inplace=True, return_info=False):
    """Tables of the altered segments of every cell (``groupby=None``) or of every group of cells.

    A segment is a maximal run of windows with the same call, -1 (loss) or +1 (gain), inside one chromosome.  Requires
    running :func:`infercnvpy_amd.tl.cnv_states` first.

    Parameters
    ----------
    adata
        annotated data matrix
    groupby
        None: one row per segment of every cell.  A column of ``adata.obs`` (``"cnv_leiden"``): the cells of every
        group vote per window, and the segments are those of the group's consensus calls.  The groups are the
        categories of a categorical column (an unused category is a group of no cells), otherwise the distinct values
        in order of appearance; cells with a missing label belong to no group and are not read.
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` is the int8 n x W matrix of -1 / 0 / +1: a host numpy array (uploaded once) or a
        CUDA int8 tensor (read where it lies), what ``tl.cnv_states`` leaves.  It never comes back to the host.
    cnv_key
        ``adata.uns[cnv_key]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        ``adata.uns[key_added]`` receives a dict: ``"segments"`` (the DataFrame), ``"params"`` and, with ``groupby``,
        ``"groups"`` (the labels), ``"n_cells"`` (int64 per group), ``"consensus"`` (int8 G x W), ``"loss"`` and
        ``"gain"`` (int32 G x W: the cells of the group with that call at the window).
    min_fraction
        in (0, 1]: a group's consensus call at a window is +1 (-1) when at least
        ``max(1, ceil(min_fraction * n_cells))`` of its cells have it and more cells than have the opposite call.  The
        product is formed exactly (``fractions.Fraction``).
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
    ``(DataFrame, consensus, loss, gain)`` of host arrays, followed by the info dict when ``return_info``.

    Per cell the columns are ``cell`` (int64 row number), ``chromosome``, ``start``, ``end`` (int32 window numbers,
    ``end`` exclusive), ``state`` (int8), ``n_windows`` (int32), ordered by (cell, start).  Per group they are
    ``group`` (the label), ``chromosome``, ``start``, ``end``, ``state``, ``n_windows``, ``n_cells`` (int64, the group's
    size), ``cells_min`` (int32, the fewest cells that have the call at any window of the segment) and ``support``
    (float64: the mean share of the group's cells that have it), ordered by (group, start).  A value other than
    -1 / 0 / +1 raises ``ValueError`` (one flag read back from the device).
    """
    import pandas as pd

    key = f"X_{use_rep}"
    x, _, _, w = call_matrix(adata, "tl.cnv_segments", key, cnv_key,
                             "`tl.cnv_states`? (it reads what `tl.infercnv` leaves there)")
    chr_pos = adata.uns[cnv_key]["chr_pos"]
    bounds = chromosome_bounds(chr_pos, w)
    fraction = unit_fraction("tl.cnv_segments", "min_fraction", min_fraction)
    shortest = at_least_one("tl.cnv_segments", "min_windows", min_windows)
    params = {"groupby": groupby, "use_rep": use_rep, "min_fraction": float(fraction), "min_windows": shortest}
    if groupby is not None:
        if groupby not in adata.obs.columns:
            raise ValueError(f"tl.cnv_segments: `{groupby}` not found in `adata.obs`"
                             + (". Did you run `tl.leiden`?" if groupby == "cnv_leiden" else ""))
        codes, groups = group_codes(adata, groupby)
        n_groups = len(groups)
        rows, group_ptr, n_cells = group_table(codes, n_groups)
        need = np.asarray([max(1, math.ceil(fraction * int(c))) for c in n_cells], dtype=np.int32)

    torch = _engine._torch()
    stage_ms = {}
    t0 = time.perf_counter()
    states = _engine.dense_input(x)
    with torch.cuda.device(states.device):
        if groupby is None:
            _, _, row, start, end, state, bad = _engine.segments_tables(states, bounds)
            row, start, end, state = (v.cpu().numpy() for v in (row, start, end, state))
            if int(bad.item()):
                raise ValueError(f"tl.cnv_segments: {key} has values other than -1, 0 and +1")
            stage_ms["segments"] = (time.perf_counter() - t0) * 1e3
        else:
            loss, gain, bad = _engine.state_votes(states, rows, group_ptr)
            consensus = _engine.state_consensus(loss, gain, need)
            if int(bad.item()):
                raise ValueError(f"tl.cnv_segments: {key} has values other than -1, 0 and +1")
            t1 = time.perf_counter()
            stage_ms["votes"] = (t1 - t0) * 1e3
            if n_groups:
                _, _, row, start, end, state, _ = _engine.segments_tables(consensus, bounds)
                cells_min, cells_sum = _engine.segments_support(row, start, end, state, loss, gain)
                row, start, end, state, cells_min, cells_sum = (
                    v.cpu().numpy() for v in (row, start, end, state, cells_min, cells_sum))
            else:
                row, cells_sum = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
                start, end, cells_min = (np.zeros(0, dtype=np.int32) for _ in range(3))
                state = np.zeros(0, dtype=np.int8)
            consensus, loss, gain = consensus.cpu().numpy(), loss.cpu().numpy(), gain.cpu().numpy()
            stage_ms["segments"] = (time.perf_counter() - t1) * 1e3

    n_segments = int(row.shape[0])
    n_windows = (end - start).astype(np.int32)
    keep = n_windows >= shortest
    columns = {"cell" if groupby is None else "group": row if groupby is None else groups[row],
               "chromosome": _chromosome_names(chr_pos, start), "start": start, "end": end, "state": state,
               "n_windows": n_windows}
    if groupby is not None:
        size = n_cells[row]
        columns["n_cells"] = size
        columns["cells_min"] = cells_min
        columns["support"] = cells_sum.astype(np.float64) / (n_windows.astype(np.int64) * size).astype(np.float64)
    table = pd.DataFrame({k: v[keep] for k, v in columns.items()})
    info = {"n_segments": n_segments, "n_groups": n_groups if groupby is not None else 0, "stage_ms": stage_ms}

    result = (table,) if groupby is None else (table, consensus, loss, gain)
    if inplace:
        out = {"segments": table, "params": params}
        if groupby is not None:
            out.update(groups=groups, n_cells=n_cells, consensus=consensus, loss=loss, gain=gain)
        adata.uns[key_added] = out
    if return_info:
        return (*result, info)
    if inplace:
        return None
    return table if groupby is None else result

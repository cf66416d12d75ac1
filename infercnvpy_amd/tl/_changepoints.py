"""tl.cnv_changepoints: piecewise-constant levels and breakpoints of ``X_cnv`` (no counterpart in the reference, which
wraps R ``copykat`` for the question).

``tl.cnv_states`` and what builds on it say *which* windows are lost or gained, with one amplitude for all of them; they
cannot say *how much*.  Here every chromosome of every row is segmented into constant levels by penalised least squares
(optimal partitioning with the L2 cost): the segmentation that minimises the residual sum of squares plus ``beta`` per
segment, found exactly by dynamic programming on the GPU by the written contract of DESIGN.md 4.19.  Float64 adds,
multiplies, divisions and compares in a fixed order: the result is a pure function of
(matrix, chr_pos, penalty, sigma, min_windows) and equals ``tests/_changepoint_oracle.py`` bit for bit.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine, _lib
from ._hmm import _positive, at_least_one, chromosome_bounds
from ._segments import _chromosome_names

WHO = "tl.cnv_changepoints"


def _penalty(value):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{WHO}: penalty={value!r} must be a number") from None
    if isinstance(value, bool) or not (math.isfinite(v) and v >= 0):
        raise ValueError(f"{WHO}: penalty={value!r} must be finite and >= 0")
    return v


def default_sigma(d_rows, n, w, n_chr):
    """Rule 6: ``sqrt(D / (2 M))`` with ``D = fsum`` of the per-row sums of squared differences and ``M = n (W - C)`` the
    number of adjacent pairs; 0.0 when there is no pair.  ``inf`` when ``D`` overflows."""
    pairs = int(n) * (int(w) - int(n_chr))
    if pairs == 0:
        return 0.0
    try:
        total = math.fsum(d_rows)
    except OverflowError:
        return math.inf
    return math.sqrt(total / (2.0 * float(pairs)))


def segments_table(levels, starts, chr_pos):
    """The per-segment table from the device tensors ``levels`` (float64 n x W) and ``starts`` (uint8 n x W): the nonzero
    positions of ``starts`` in row-major order are the segment starts, a segment ends at the next start of its row or at
    W, its mean is ``levels`` at its start.  One copy to the host."""
    import pandas as pd

    torch = _engine._torch()
    w = int(starts.shape[1])
    at = torch.nonzero(starts)  # (K, 2) int64, row-major
    row, start = at[:, 0], at[:, 1]
    end = torch.full_like(start, w)
    if int(at.shape[0]) > 1:
        end[:-1] = torch.where(row[1:] == row[:-1], start[1:], end[:-1])
    mean = levels[row, start]
    host = torch.stack([row, start, end, mean.view(torch.int64)], dim=1).cpu().numpy()
    start_h, end_h = host[:, 1].astype(np.int32), host[:, 2].astype(np.int32)
    return pd.DataFrame({"cell": host[:, 0].copy(), "chromosome": _chromosome_names(chr_pos, start_h), "start": start_h,
                         "end": end_h, "n_windows": (end_h - start_h).astype(np.int32),
                         "mean": host[:, 3].copy().view(np.float64)})


def cnv_changepoints(adata, use_rep="cnv", key_added="cnv_levels", *, penalty=2.0, sigma=None, min_windows=1, table=True,
                     inplace=True, return_info=False):
    """Segment every chromosome of every row into constant levels: the exact penalised least-squares change points.

    For each row and chromosome the windows are split into segments so that the sum of squared deviations from the
    segment means plus ``beta`` per segment is smallest (optimal partitioning, solved exactly by dynamic programming on
    the GPU); every window gets its segment's mean.  Unlike :func:`infercnvpy_amd.tl.cnv_states` the levels are not tied to
    one amplitude: a one-copy gain at +0.3 and a two-copy gain at +0.6 come out as different levels, and a high-level
    amplification next to a low-level gain as two segments.  Segments never cross a chromosome boundary.  Requires
    running :func:`infercnvpy_amd.tl.infercnv` first; it runs on the clone profiles of
    :func:`infercnvpy_amd.tl.cnv_pseudobulk` as well::

        clones = cnv.tl.cnv_pseudobulk(adata, "cnv_leiden")
        cnv.tl.cnv_changepoints(clones)
        clones.uns["cnv_levels"]["segments"]  # one row per segment of every clone, with its mean

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) is segmented: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, float32 or float64.  Stored values are used as float64,
        an entry that is not stored is 0.0.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every
        chromosome; a chromosome has at most 4 096 windows.
    key_added
        The levels go to ``adata.obsm[f"X_{key_added}"]`` (float64), the number of segments of every row to
        ``adata.obs[key_added + "_n_segments"]`` (int32), and ``adata.uns[key_added]`` receives ``"chr_pos"`` (a copy, so
        ``pl.chromosome_heatmap(adata, use_rep=key_added)`` and ``tl.cnv_states(adata, use_rep=key_added)`` work
        unchanged), ``"params"`` (``penalty``, ``sigma``, ``beta``, ``min_windows``), ``"use_rep"`` and, with ``table``,
        ``"segments"``.
    penalty
        finite and >= 0.  A segment costs ``beta = penalty * sigma^2 * log(W)``; 2.0 is the BIC-like choice that keeps
        pure noise in one piece.  0 splits wherever it lowers the residual at all.
    sigma
        Standard deviation of the noise; None: the difference-based estimate ``sqrt(D / (2 M))``, D the exactly rounded
        sum (``math.fsum``) of the per-row sums of ``(x[t + 1] - x[t])^2`` over the adjacent windows of every chromosome
        (formed on the device), M their number.  Unlike the root mean square of ``tl.cnv_states`` it does not count the
        level shifts themselves as noise.
    min_windows
        The fewest windows of a segment (an integer >= 1); a chromosome of fewer windows is one segment.
    table
        Also build the DataFrame of segments: ``cell`` (int64 row number), ``chromosome``, ``start``, ``end`` (int32
        window numbers, ``end`` exclusive), ``n_windows`` (int32), ``mean`` (float64), ordered by (cell, start): the
        columns of ``tl.cnv_segments``' per-cell table with ``mean`` in place of ``state``.
    inplace
        If True, store the result in adata, otherwise return ``(levels, starts)`` and write nothing; ``starts`` (uint8
        n x W) is 1 at the first window of every segment.
    return_info
        Also return a dict: ``sigma``, ``beta``, ``n_chromosomes``, ``longest_chromosome`` and ``stage_ms`` (checks and
        sigma, levels, table; host clocks, the second one waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(levels, starts)``, followed by the info dict when
    ``return_info``.  Host input gives host numpy arrays, device input (``PackedCsr``, CUDA tensor) leaves both on the
    device as CUDA tensors.  A non-finite value raises ``ValueError`` (one flag read back from the device before the
    segmentation is launched), and so does a finite one so large that the sums of squares of a chromosome could overflow:
    with ``a`` the largest magnitude, ``(a a) W``, ``(a W) (a W)`` and ``beta W`` must be finite.
    """
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{WHO}: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"{WHO}: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    x = adata.obsm[key]
    if len(x.shape) != 2:
        raise ValueError(f"{WHO}: X must be 2-D")
    n, w = int(x.shape[0]), int(x.shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{WHO}: empty matrix of shape {(n, w)}")
    chr_pos = adata.uns[use_rep]["chr_pos"]
    bounds = chromosome_bounds(chr_pos, w, WHO)
    n_chr = int(bounds.shape[0]) - 1
    longest = int(np.diff(bounds).max())
    cap = _lib.ICV_CHANGEPOINT_MAX_CHR_WINDOWS
    if longest > cap:
        raise ValueError(f"{WHO}: a chromosome of {longest} windows; the kernel keeps one chromosome in LDS and takes at "
                         f"most {cap} windows")
    pen = _penalty(penalty)
    sig = None if sigma is None else _positive("sigma", sigma, WHO)
    shortest = at_least_one(WHO, "min_windows", min_windows)

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    dm = _engine.matrix_input(x, WHO)
    t0 = time.perf_counter()
    with torch.cuda.device(dm.device):
        _, flag = _engine.states_rowsq(dm)
        absmax = _engine.states_absmax(_engine.states_stored_values(dm))
        if sig is None:
            d_host = _engine.changepoint_diffsq(dm, bounds).cpu().numpy()
        nonfinite, a = _engine.flag_and_absmax(flag, absmax)
        if nonfinite:
            raise ValueError(f"{WHO}: {key} has non-finite values")
        if sig is None:
            sig = default_sigma(d_host.tolist(), n, w, n_chr)
            if not math.isfinite(sig):
                raise ValueError(f"{WHO}: the default sigma of {key} overflows float64; pass sigma")
        beta = (pen * (sig * sig)) * math.log(w)

        def overflows(v):
            t = v * float(w)
            return not (math.isfinite((v * v) * float(w)) and math.isfinite(t * t))

        if overflows(a) and isinstance(x, _engine.PackedCsr):  # (the unused tail of its buffers was looked at too)
            a = float(_engine.states_absmax(x.data[:x.nnz()]).item())
        if overflows(a):
            raise ValueError(f"{WHO}: the value of magnitude {a!r} in {key} overflows float64 over {w} windows: "
                             "(a a) W and (a W) (a W) must be finite; rescale the matrix or clip the value")
        if not math.isfinite(beta * float(w)):
            raise ValueError(f"{WHO}: penalty={pen!r} and sigma={sig!r} overflow float64: beta W = "
                             f"penalty sigma^2 log(W) W must be finite")
        t1 = time.perf_counter()
        levels, starts, count = _engine.changepoint_levels(dm, bounds, beta=beta, min_windows=shortest)
        stage_ms = {"sigma": (t1 - t0) * 1e3}
        if return_info:
            torch.cuda.current_stream().synchronize()
            stage_ms["levels"] = (time.perf_counter() - t1) * 1e3
        segments = None
        if inplace:
            if table:
                t2 = time.perf_counter()
                segments = segments_table(levels, starts, chr_pos)
                stage_ms["table"] = (time.perf_counter() - t2) * 1e3
            count = count.cpu().numpy()
        if not on_device:
            levels, starts = levels.cpu().numpy(), starts.cpu().numpy()
    info = {"sigma": sig, "beta": beta, "n_chromosomes": n_chr, "longest_chromosome": longest, "stage_ms": stage_ms}
    if inplace:
        adata.obsm[f"X_{key_added}"] = levels
        adata.obs[key_added + "_n_segments"] = count
        out = {"chr_pos": dict(chr_pos), "params": {"penalty": pen, "sigma": sig, "beta": beta, "min_windows": shortest},
               "use_rep": use_rep}
        if table:
            out["segments"] = segments
        adata.uns[key_added] = out
        return (levels, starts, info) if return_info else None
    return (levels, starts, info) if return_info else (levels, starts)

"""The contract of the ``calculate_gene_values`` layer from the plan's run tables, in numpy.

``GenePlan.gene_runs()`` says which windows a gene's value averages: run ``r`` covers ``genes[r]`` genes and averages the
windows ``[first[r], first[r] + count[r])``; ``col_run[c]`` is the run of input column ``c`` (-1: no value).  From
identical float64 windows the layer is then pure numpy and the kernels (``k_gene_fused``; ``k_gene_means`` ->
``k_row_median`` -> ``k_gene_finish``) must reproduce it bit for bit: numpy's sum order, one correctly rounded division, an
exact order statistic, ``(v1 + v2) / 2.0``, one subtraction and one compare.

Two clauses bound the contract:

* the sign of a zero is outside it (the kernels start their sums from +0.0, numpy's start depends on its version):
  :func:`same_bytes` compares ``x + 0.0``;
* the windows are finite or NaN.  A row with a NaN window in any run is NaN in every covered column (``np.median``);
  +-inf windows are not part of it.

:func:`median_path` and :func:`row_median_path` restate the SEARCHES of the two median kernels on the host.  They are
never used for expected values: they only prove that a planted case reaches the branch it is named for.
"""
import numpy as np

GV_BINS = 2048   # kGvBins
GV_CAND = 64     # kGvCand
RM_CAND = 1024   # k_row_median's candidate buffer
RM_VALUE_ITERS = 60  # k_row_median: value-space bisection before the key-space one


def run_values(runs, w):
    """val[r] of one row of windows: np.mean of the run's windows, as numpy forms it."""
    first, count = np.asarray(runs["first"]), np.asarray(runs["count"])
    val = np.empty(len(first), dtype=np.float64)
    one = count == 1  # (the sum of one element is that element: no Python loop over the rows of the planted plans)
    val[one] = w[first[one]] / 1.0
    for r in np.flatnonzero(~one):
        val[r] = np.add.reduce(np.ascontiguousarray(w[first[r]:first[r] + count[r]])) / count[r]
    return val


def gene_layer(runs, windows, n_cols, thr=None, chunksize=1, row_phase=0):
    """float64 ``rows x n_cols`` layer of ``windows`` (rows x W float64) under the run tables ``runs``."""
    windows = np.asarray(windows, dtype=np.float64)
    genes, col_run = np.asarray(runs["genes"]), np.asarray(runs["col_run"])
    assert col_run.shape == (n_cols,)
    has = col_run >= 0
    out = np.full((windows.shape[0], n_cols), np.nan)
    for row in range(windows.shape[0]):
        val = run_values(runs, windows[row])
        with np.errstate(invalid="ignore"):
            med = np.median(np.repeat(val, genes))
            a = val - med
            if thr is not None:
                a[np.abs(a) < thr[(row + row_phase) // chunksize]] = 0.0
        out[row, has] = a[col_run[has]]
    return out


def same_bytes(got, want):
    """NaN masks identical, every other value identical in all 64 bits after ``+ 0.0`` (the sign of a zero is outside
    the contract).  Nothing else is normalised; there is no tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and want.dtype == np.float64 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    np.testing.assert_array_equal(gn, wn)
    g = np.where(gn, 0.0, got) + 0.0
    w = np.where(wn, 0.0, want) + 0.0
    bad = np.flatnonzero(g.view(np.int64).ravel() != w.view(np.int64).ravel())
    if bad.size:
        i = np.unravel_index(bad[0], got.shape)
        raise AssertionError(f"{bad.size} of {got.size} values differ in their bits; first at {i}: "
                             f"got {got[i]!r} ({got[i].hex()}), want {want[i]!r} ({want[i].hex()})")


def _bins(v, lo, hi):
    """The fused kernel's bin of every v in [lo, hi]: min(int((v - lo) * (2048 / (hi - lo))), 2047).  Where hi - lo is so
    small that the quotient overflows, (v - lo) * inf is NaN for v == lo and inf above: the conversion gives 0 and
    saturates (the clamp)."""
    with np.errstate(over="ignore", invalid="ignore"):
        scale = np.float64(GV_BINS) / (np.float64(hi) - np.float64(lo))
        x = (v - lo) * scale
    x = np.where(np.isnan(x), 0.0, np.minimum(x, float(GV_BINS)))
    return np.minimum(x.astype(np.int64), GV_BINS - 1)


def median_path(val, genes):
    """Host restatement of the weighted-median search of ``k_gene_fused`` over the multiset {val[r] x genes[r]}.

    -> dict(counts=[run values in the selected bin, per level], bins=[selected bin per level],
            end="candidates" | "equal" | "candidates+next_above" | "equal+next_above", v1, v2)
    ``counts`` has one entry per histogram level; an "equal" ending adds no entry (it happens on entering a level, so
    ``len(counts)`` IS the level it happened at)."""
    val, genes = np.asarray(val, dtype=np.float64), np.asarray(genes, dtype=np.int64)
    assert not np.isnan(val).any() and len(val) == len(genes) and len(val) > 0
    n_cov = int(genes.sum())
    k1, k2 = (n_cov - 1) // 2, n_cov // 2
    lo, hi = val.min(), val.max()
    below, need2 = 0, k2 != k1
    counts, bins, end, v1, v2 = [], [], None, lo, lo
    for _level in range(64):
        if not hi > lo:
            v1 = lo
            wt = int(genes[val == lo].sum())
            if need2 and k2 - below < wt:
                v2, need2 = lo, False
            end = "equal"
            break
        inr = (val >= lo) & (val <= hi)
        b = _bins(val[inr], lo, hi)
        hist = np.bincount(b, weights=genes[inr], minlength=GV_BINS).astype(np.int64)
        cum = np.cumsum(hist)
        sb = int(np.searchsorted(cum, k1 - below, side="right"))
        below += int(cum[sb] - hist[sb])
        sel_v, sel_w = val[inr][b == sb], genes[inr][b == sb]
        counts.append(len(sel_v))
        bins.append(sb)
        if len(sel_v) <= GV_CAND:
            order = np.argsort(sel_v, kind="stable")
            sv, cw = sel_v[order], np.cumsum(sel_w[order])
            v1 = sv[np.searchsorted(cw, k1 - below, side="right")]
            if need2 and k2 - below < cw[-1]:
                v2, need2 = sv[np.searchsorted(cw, k2 - below, side="right")], False
            end = "candidates"
            break
        lo, hi = sel_v.min(), sel_v.max()
    assert end is not None, "no ending within 64 levels"
    if need2:
        v2 = val[val > v1].min()
        end += "+next_above"
    elif k1 == k2:
        v2 = v1
    return dict(counts=counts, bins=bins, end=end, v1=float(v1), v2=float(v2))


def _key(x):
    b = int(np.float64(x).view(np.uint64))
    return (~b & 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b | 0x8000000000000000)


def _from_key(k):
    b = (k & 0x7FFFFFFFFFFFFFFF) if k >> 63 else (~k & 0xFFFFFFFFFFFFFFFF)
    return np.uint64(b).view(np.float64)


def row_median_path(x):
    """Host restatement of the search of ``k_row_median`` over one row ``x`` (the covered genes' values).

    -> dict(iters=bisection steps taken, end="separated" | "adjacent" | "candidates", key_space=steps taken on the keys)"""
    x = np.asarray(x, dtype=np.float64)
    assert not np.isnan(x).any() and len(x) > 0
    n = len(x)
    k1, k2 = (n - 1) // 2, n // 2
    mn = x.min()
    lo = np.float64(-5e-324) if mn == 0.0 else np.nextafter(mn, -np.inf)
    hi = x.max()
    cnt_lo, cnt_hi, it, key_space = 0, n, 0, 0
    while cnt_hi - cnt_lo > RM_CAND and it < 200:
        if it < RM_VALUE_ITERS:
            mid = np.float64(0.5) * lo + np.float64(0.5) * hi
        else:
            a, b = _key(lo), _key(hi)
            mid = _from_key(a + ((b - a) >> 1))
        if not (mid > lo and mid < hi):
            break
        key_space += it >= RM_VALUE_ITERS
        c = int((x <= mid).sum())
        if c > k2:
            hi, cnt_hi = mid, c
        elif c <= k1:
            lo, cnt_lo = mid, c
        else:
            return dict(iters=it + 1, end="separated", key_space=key_space)
        it += 1
    end = "adjacent" if cnt_hi - cnt_lo > RM_CAND else "candidates"
    return dict(iters=it, end=end, key_space=key_space)

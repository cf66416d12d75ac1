"""The written contract of tl.cnv_correlation and tl.cnv_signal in numpy: a loop over the windows,
vectorised over cells and profiles.

  1. host, float64: m_g = fsum(p_g) / W, c_g = p_g - m_g, s2_g = fsum(c_g c_g).
  2. per cell, sequentially over the windows in ascending order, from +0.0: A += x, B += x x, D_g += x c_g[w]; every
     product is rounded before its add.  An entry that is not stored is 0 and adds nothing.
  3. vx = B - (A A) / W; r_g = D_g / sqrt(vx s2_g), clipped to [-1, 1]; NaN where vx <= 0 or s2_g == 0; signal = B / W.
  4. best = the lowest g with the largest r that is no NaN; -1 and NaN when the whole row is NaN.
"""
import fractions
import math

import numpy as np
import scipy.sparse as sp

import _pseudobulk_oracle as pb


def centre(p):
    """(c G x W, s2 G) of rule 1 for G x W float64 profiles."""
    p = np.asarray(p, dtype=np.float64)
    g_count, w = p.shape
    c = np.empty((g_count, w), dtype=np.float64)
    s2 = np.empty(g_count, dtype=np.float64)
    for g in range(g_count):
        m = math.fsum(p[g].tolist()) / w
        c[g] = p[g] - m
        s2[g] = math.fsum((c[g] * c[g]).tolist())
    return c, s2


def windows(x):
    """The n x W float64 array of the matrix: an entry that is not stored is +0.0, duplicates of a sparse matrix are
    merged as scipy's canonical format does."""
    if sp.issparse(x):
        x = x.tocsr().toarray()
    return np.asarray(x).astype(np.float64)


def sums(x, c):
    """(A, B, D) of rule 2: one pass over the windows in ascending order."""
    d = windows(x)
    n, w = d.shape
    A, B, D = np.zeros(n), np.zeros(n), np.zeros((n, c.shape[0]))
    for j in range(w):
        v = d[:, j]
        A = A + v
        B = B + v * v
        D = D + v[:, None] * c[:, j][None, :]
    return A, B, D


def finish(A, B, D, s2, w):
    """(signal, r) of rule 3."""
    with np.errstate(all="ignore"):
        vx = B - (A * A) / float(w)
        r = D / np.sqrt(vx[:, None] * s2[None, :])
        r = np.where(r > 1.0, 1.0, np.where(r < -1.0, -1.0, r))
        r = np.where((vx[:, None] > 0.0) & (s2[None, :] != 0.0), r, np.nan)
        return B / float(w), r


def best(r):
    """(best_r float64, best_g int32) of rule 4."""
    n, g_count = r.shape
    best_r, best_g = np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
    for g in range(g_count):
        v = r[:, g]
        with np.errstate(invalid="ignore"):
            take = ~np.isnan(v) & ((best_g < 0) | (v > best_r))
        best_r[take], best_g[take] = v[take], g
    return best_r, best_g


def correlate(x, p):
    """dict(A, B, signal, r, best_r, best_g) of the rows of ``x`` against the G x W profiles ``p`` (G may be 0)."""
    d = windows(x)
    p = np.asarray(p, dtype=np.float64).reshape(-1, d.shape[1])
    c, s2 = centre(p)
    A, B, D = sums(d, c)
    signal, r = finish(A, B, D, s2, d.shape[1])
    best_r, best_g = best(r)
    return {"A": A, "B": B, "signal": signal, "r": r, "best_r": best_r, "best_g": best_g}


def top_count(top_fraction, n):
    """k = max(1, ceil(top_fraction n)), the product formed exactly."""
    return max(1, math.ceil(fractions.Fraction(top_fraction) * n))


def top_rows(signal, top_fraction):
    """The ascending int64 rows of the k cells of largest signal, ties going to the lower row."""
    signal = np.asarray(signal, dtype=np.float64)
    k = top_count(top_fraction, signal.shape[0])
    order = sorted(range(signal.shape[0]), key=lambda i: (-signal[i], i))
    return np.asarray(sorted(order[:k]), dtype=np.int64)


def top_profile(x, top_fraction):
    """(rows, 1 x W mean profile of those rows by the contract of tl.cnv_pseudobulk) of the "top" mode."""
    d = windows(x)
    rows = top_rows(correlate(d, np.zeros((0, d.shape[1])))["signal"], top_fraction)
    codes = np.full(d.shape[0], -1, dtype=np.int64)
    codes[rows] = 0
    return rows, pb.profiles(x, codes, 1)["mean"]


def same_bytes(a, b):
    """Equal float64 bytes, a NaN equal to a NaN at the same position whatever its payload."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb]))


# ---- the planted case of DESIGN.md 4.18 ----------------------------------------------------------------------------------------
def planted(seed):
    """3 clones x 48 tumour cells that share a trunk event and have a private one each, plus 96 normal cells; 270 windows,
    noise 0.3, shifts of +-0.3, rows permuted.  dict(x dense float64, clone int64 per row (-1 = normal), truth 3 x 270)."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((3, 270))
    truth[:, 20:55] = 0.3      # the trunk: a gain and a loss
    truth[:, 140:175] = -0.3
    truth[0, 65:105] = -0.3    # one private event per clone
    truth[1, 185:225] = 0.3
    truth[2, 225:265] = -0.3
    clone = np.concatenate([np.repeat(np.arange(3), 48), np.full(96, -1)])[rng.permutation(240)]
    x = rng.normal(0.0, 0.3, (240, 270))
    tumour = clone >= 0
    x[tumour] += truth[clone[tumour]]
    return {"x": x, "clone": clone.astype(np.int64), "truth": truth}

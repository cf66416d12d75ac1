"""numpy oracle of tl.umap: DESIGN.md 4.11 restated (the specification; umap-learn is not available).

A gather ("Jacobi") form of umap-learn's ``optimize_layout_euclidean``: every vertex is updated from the same snapshot
of the previous epoch, so the layout is a pure function of (graph, parameters, random_state, initial positions).

1. Graph: canonical symmetric CSR, data rounded to float32.  Entry e is its position in the CSR.
2. Schedule (float64, stateless): w_max = the largest weight, p_e = w_max / w_e.  Entries with w_e = 0 or
   w_e < w_max / n_epochs never fire.  c(t) = floor(t / p_e); e is active in epoch t iff t >= 1 and c(t) > c(t - 1).
3. Active entry (i, j): d = y_i - y_j (float64 of the float32 positions), d2 = sum of d^2 left to right,
   pb = pow(d2, b), coeff = ((-2 a) b (pb / d2)) / (a pb + 1) when d2 > 0 else 0; contribution 2 clip(coeff d, -4, 4).
4. Negatives: s = 0 .. r - 1 per active entry, k = ((h >> 32) n) >> 32 with h = mix(mix(seed ^ mix(t)) ^ (e r + s));
   0 when k == i or d2 == 0, else clip(((2 gamma) b / ((0.001 + d2) (a pb + 1))) (y_i - y_k), -4, 4).
5. Every per-coordinate contribution v becomes the int64 rint(v 2^32); a row's contributions are added as integers.
6. alpha_t = initial_alpha (1 - t / n_epochs); y_i <- float32(float64(y_i) + alpha_t (S_i 2^-32)) for the rows with an
   active entry, the others keep their position.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

MASK = (1 << 64) - 1
TAG_RANDOM = MASK       # the "epoch" of the random initial positions
TAG_NOISE = MASK - 1    # ... of the noise added to the spectral ones


def mix_int(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def mix(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def counter_hash(seed, t, counters):
    """mix(mix(seed ^ mix(t)) ^ counter) for a uint64 array of counters."""
    base = mix_int((seed & MASK) ^ mix_int(t))
    return mix(np.uint64(base) ^ np.asarray(counters, dtype=np.uint64))


def uniform24(seed, tag, n, c):
    """n x c float64 numbers k / 2^24, k the top 24 bits of the counter hash of (tag, i c + j)."""
    h = counter_hash(seed, tag, np.arange(n * c, dtype=np.uint64))
    return ((h >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).reshape(n, c)


def random_init(n, c, seed):
    """init_pos="random": uniform in [-10, 10)."""
    return (uniform24(seed, TAG_RANDOM, n, c) * 20.0 - 10.0).astype(np.float32)


def find_ab(spread=1.0, min_dist=0.5):
    """umap-learn's find_ab_params."""
    from scipy.optimize import curve_fit

    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    return float(a), float(b)


A_DEFAULT, B_DEFAULT = 0.5830300203414425, 1.3341669924314914  # find_ab(1.0, 0.5), for tests that need no scipy fit


class Graph:
    def __init__(self, graph):
        g = sp.csr_matrix(graph)
        if g is graph:
            g = g.copy()
        g.sum_duplicates()
        g.sort_indices()
        self.n = g.shape[0]
        self.indptr = g.indptr.astype(np.int64)
        self.indices = g.indices.astype(np.int64)
        self.w = g.data.astype(np.float32).astype(np.float64)
        self.rows = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.indptr))
        self.w_max = float(self.w.max()) if len(self.w) else 0.0

    def fires(self, n_epochs):
        """The entries that ever fire in an n_epochs schedule (rule 2)."""
        return (self.w > 0) & (self.w >= self.w_max / n_epochs)

    def active(self, t, n_epochs):
        """Indices of the entries active in epoch t."""
        if t < 1:
            return np.zeros(0, dtype=np.int64)
        e = np.flatnonzero(self.fires(n_epochs))
        p = self.w_max / self.w[e]
        return e[np.floor(t / p) > np.floor((t - 1) / p)]


def _pair(y64, i, j, b):
    d = y64[i] - y64[j]
    d2 = d[:, 0] * d[:, 0]
    for q in range(1, d.shape[1]):
        d2 = d2 + d[:, q] * d[:, q]
    with np.errstate(divide="ignore", invalid="ignore"):
        pb = np.power(d2, b)
    return d, d2, pb


def _quantise(v):
    return np.rint(v * 4294967296.0).astype(np.int64)


def contributions(g, y, t, *, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, seed=0):
    """(rows, q): the int64 contributions (m x c) of epoch t and the row each one goes to; 1 + r per active entry."""
    r = int(negative_sample_rate)
    e = g.active(t, n_epochs)
    i = g.rows[e]
    y64 = y.astype(np.float64)
    c = y.shape[1]
    rows, qs = [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        d, d2, pb = _pair(y64, i, g.indices[e], b)
        coeff = np.where(d2 > 0, ((-2.0 * a) * b * (pb / d2)) / (a * pb + 1.0), 0.0)
        rows.append(i)
        qs.append(_quantise(2.0 * np.clip(coeff[:, None] * d, -4.0, 4.0)))
        for s in range(r):
            h = counter_hash(seed, t, e.astype(np.uint64) * np.uint64(r) + np.uint64(s))
            k = (((h >> np.uint64(32)) * np.uint64(g.n)) >> np.uint64(32)).astype(np.int64)
            d, d2, pb = _pair(y64, i, k, b)
            coeff = np.where((d2 > 0) & (k != i), ((2.0 * gamma) * b) / ((0.001 + d2) * (a * pb + 1.0)), 0.0)
            rows.append(i)
            qs.append(_quantise(np.clip(coeff[:, None] * d, -4.0, 4.0)))
    return np.concatenate(rows), np.concatenate(qs).reshape(-1, c)


def epoch(g, y, t, *, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, initial_alpha=1.0, seed=0, order=None):
    """(y_new, m): one epoch from the snapshot y (float32 n x c); m[i] = contributions of row i.  `order`: a
    permutation of the contributions (the sum does not depend on it)."""
    rows, q = contributions(g, y, t, n_epochs=n_epochs, a=a, b=b, gamma=gamma,
                            negative_sample_rate=negative_sample_rate, seed=seed)
    if order is not None:
        rows, q = rows[order], q[order]
    S = np.zeros(y.shape, dtype=np.int64)
    np.add.at(S, rows, q)
    m = np.bincount(rows, minlength=g.n)
    alpha = initial_alpha * (1.0 - t / n_epochs)
    new = (y.astype(np.float64) + alpha * (S.astype(np.float64) * 2.0 ** -32)).astype(np.float32)
    return np.where((m > 0)[:, None], new, y), m


def run(g, y, epoch_begin, epoch_end, keep=(), **kw):
    """The epochs [epoch_begin, epoch_end); `keep`: epochs t whose snapshot (the positions BEFORE epoch t) is returned
    as well, as a dict."""
    snaps = {}
    y = np.ascontiguousarray(y, dtype=np.float32)
    for t in range(epoch_begin, epoch_end):
        if t in keep:
            snaps[t] = y
        y, _ = epoch(g, y, t, **kw)
    return (y, snaps) if keep else y


# ---- the quality measure ----------------------------------------------------------------------------------------------
def neighbour_preservation(graph_knn, y, k, rows=None, block=256):
    """Mean fraction of a row's k input neighbours (graph_knn: n x >= k indices, without the row itself) that are among
    its k nearest points in the layout y; over `rows` (default: all)."""
    y = np.asarray(y, dtype=np.float64)
    rows = np.arange(len(y)) if rows is None else np.asarray(rows)
    sq = (y * y).sum(1)
    hit = 0
    for s in range(0, len(rows), block):
        rr = rows[s:s + block]
        d = sq[rr][:, None] + sq[None, :] - 2.0 * (y[rr] @ y.T)
        d[np.arange(len(rr)), rr] = -np.inf
        nn = np.argpartition(d, k, axis=1)[:, :k + 1]  # the row itself and its k nearest; graph_knn has no self
        for a, bb in zip(nn, graph_knn[rr, :k]):
            hit += len(np.intersect1d(a, bb))
    return hit / (len(rows) * k)

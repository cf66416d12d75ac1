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


def contributions(g, y, t, *, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, seed=0, drop=None):
    """(rows, q): the int64 contributions (m x c) of epoch t and the row each one goes to; 1 + r per active entry.
    `drop`: entries treated as inactive (what a kernel that loses them would compute; the others keep their samples)."""
    r = int(negative_sample_rate)
    e = g.active(t, n_epochs)
    if drop is not None:
        e = e[~np.isin(e, drop)]
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


def epoch(g, y, t, *, n_epochs, a, b, gamma=1.0, negative_sample_rate=5, initial_alpha=1.0, seed=0, order=None,
          drop=None):
    """(y_new, m): one epoch from the snapshot y (float32 n x c); m[i] = contributions of row i.  `order`: a
    permutation of the contributions (the sum does not depend on it); `drop`: see :func:`contributions`."""
    rows, q = contributions(g, y, t, n_epochs=n_epochs, a=a, b=b, gamma=gamma,
                            negative_sample_rate=negative_sample_rate, seed=seed, drop=drop)
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


def tolerance(ref, m):
    """The bound of a one-epoch comparison with :func:`epoch`'s (ref, m).  Derived, not measured: pow may differ in its
    last bit, which moves a contribution to the neighbouring multiple of 2^-32 (m_i contributions, alpha <= 1), and
    then the final float32 rounding may fall to the other side."""
    return np.spacing(np.abs(ref)).astype(np.float64) + m[:, None] * 2.0 ** -32


def negatives(g, y, t, *, n_epochs, negative_sample_rate=5, seed=0):
    """(i, k, d2) of every negative sample of epoch t (rule 4): the row, the sampled vertex and their squared distance."""
    r = int(negative_sample_rate)
    e = g.active(t, n_epochs)
    c = (e.astype(np.uint64)[:, None] * np.uint64(r) + np.arange(r, dtype=np.uint64)[None, :]).ravel()
    h = counter_hash(seed, t, c)
    k = (((h >> np.uint64(32)) * np.uint64(g.n)) >> np.uint64(32)).astype(np.int64)
    i = np.repeat(g.rows[e], r)
    return i, k, _pair(y.astype(np.float64), i, k, 1.0)[1]


# ---- edge builders (tests/test_gpu_umap_edges.py; test_umap_oracle.py asserts that the oracle reaches each branch) -----
CHUNK = 64      # entries a wavefront tests per ballot
LDS_ROW = 512   # longest row a wavefront compacts; longer rows take a workgroup
HUBS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 511, 512, 513, 514, 1025)


def _sym(rows, cols, vals, n):
    """Symmetric CSR of the edges (rows, cols) with float32 values; stored zeros (of either sign) are kept."""
    rows, cols, vals = np.asarray(rows), np.asarray(cols), np.asarray(vals, dtype=np.float32)
    r, c, v = np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([vals, vals])
    order = np.lexsort((c, r))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))])
    return sp.csr_matrix((v[order], c[order].astype(np.int32), indptr.astype(np.int64)), shape=(n, n))


def hubs_mixed(hubs=HUBS, leaves=1030, seed=0):
    """A path of weight 1 over `leaves` vertices plus one hub per entry d of `hubs`, joined to the leaves 0 .. d - 1 by
    weights j / 64, j uniform in [0, 64] (float32-exact; the zeros are stored).  Hub h is vertex leaves + h, so its row
    has d entries in ascending leaf order: rows on both sides of every multiple of 64 and of the 512-entry split, whose
    64-entry chunks mix active and inactive entries in most epochs."""
    rng = np.random.default_rng(seed)
    r, c, v = [np.arange(leaves - 1)], [np.arange(1, leaves)], [np.ones(leaves - 1)]
    for h, d in enumerate(hubs):
        r.append(np.arange(d))
        c.append(np.full(d, leaves + h))
        v.append(rng.integers(0, 65, d) / 64.0)
    return _sym(np.concatenate(r), np.concatenate(c), np.concatenate(v), leaves + len(hubs))


def hub_rows(g, leaves=1030):
    """The hub vertices of :func:`hubs_mixed` (every vertex from `leaves` on)."""
    return np.arange(leaves, g.shape[0])


def split_mixed(seed=1):
    """The pattern of ``_leiden_oracle.rows_at_split()``: cliques of 513, 514 and 512 vertices joined in a ring, rows of
    511 .. 514 entries (hundreds of long rows next to hundreds of short ones), with symmetric weights j / 8, j uniform
    in [0, 8]."""
    import _leiden_oracle as lo

    g = sp.coo_matrix(lo.rows_at_split())
    up = g.row < g.col
    rng = np.random.default_rng(seed)
    return _sym(g.row[up], g.col[up], rng.integers(0, 9, int(up.sum())) / 8.0, g.shape[0])


def threshold_values(n_epochs):
    """name -> float32 weight around the limits of rule 2 when w_max = 1."""
    thr = np.float32(1.0 / n_epochs)
    return {"one": np.float32(1.0), "at": thr, "above": np.nextafter(thr, np.float32(2.0)),
            "below": np.nextafter(thr, np.float32(0.0)), "zero": np.float32(0.0), "minus_zero": np.float32(-0.0),
            "third": np.float32(1.0 / 3.0), "subnormal": np.nextafter(np.float32(0.0), np.float32(1.0))}


def threshold_weights(n_epochs):
    """A star whose leaf 1 + q carries the q-th weight of :func:`threshold_values`, followed by a path of weight 1 / 3
    over four more vertices hanging off the last leaf (rows that mix a firing and a non-firing entry)."""
    w = np.array(list(threshold_values(n_epochs).values()), dtype=np.float32)
    k = len(w)
    r = np.concatenate([np.zeros(k, dtype=np.int64), np.arange(k, k + 4)])
    c = np.concatenate([np.arange(1, k + 1), np.arange(k + 1, k + 5)])
    return _sym(r, c, np.concatenate([w, np.full(4, np.float32(1.0 / 3.0))]), k + 5)


def zero_weights(n=21):
    """A path whose stored weights are all zero, of both signs: w_max = 0."""
    return _sym(np.arange(n - 1), np.arange(1, n), np.where(np.arange(n - 1) % 2, -0.0, 0.0), n)


def chunk_counts(g, v, t, n_epochs):
    """Active entries per 64-entry chunk of row v in epoch t, and the entries per chunk."""
    b, e = int(g.indptr[v]), int(g.indptr[v + 1])
    act = np.zeros(e - b, dtype=np.int64)
    a = g.active(t, n_epochs)
    act[a[(a >= b) & (a < e)] - b] = 1
    edges = np.arange(0, e - b, CHUNK)
    return np.add.reduceat(act, edges), np.diff(np.r_[edges, e - b])


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

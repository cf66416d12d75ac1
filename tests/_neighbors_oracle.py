"""numpy oracle of pp.neighbors: DESIGN.md 4.9 restated (the specification; scanpy / umap-learn are not available).

k = n_neighbors; every cell has k - 1 neighbours, itself never among them.
1. points: the float32 values as given;
2. d2(i, j) = sum over c (in order, float64, no fused multiply-add) of (double(x_ic) - double(x_jc))^2, stored
   distance = float32(sqrt(d2));
3. neighbours of i: the k - 1 cells j != i with the smallest (d2, j), in that order;
4. distances: canonical CSR with explicit zeros, k - 1 stored entries per row;
5. connectivities: UMAP's fuzzy_simplicial_set (local_connectivity = 1, set_op_mix_ratio = 1) in float64 on the
   stored float32 distances, C = A + A^T - A o A^T as float32 canonical CSR without stored zeros.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.sparse as sp


def sq_dists(x, rows):
    """float64 d2 of the rows `rows` (index array) against all cells, columns summed in order."""
    x = np.asarray(x, dtype=np.float32)
    out = np.zeros((len(rows), x.shape[0]), dtype=np.float64)
    xr = x[rows].astype(np.float64)
    for c in range(x.shape[1]):
        t = xr[:, c, None] - x[None, :, c].astype(np.float64)
        out += t * t
    return out


def _knn_block(x, rows, km1):
    dd = sq_dists(x, rows)
    dd[np.arange(len(rows)), rows] = np.inf  # the cell itself
    kth = np.partition(dd, km1 - 1, axis=1)[:, km1 - 1]
    idx = np.empty((len(rows), km1), dtype=np.int32)
    d2 = np.empty((len(rows), km1), dtype=np.float64)
    for r in range(len(rows)):
        cand = np.flatnonzero(dd[r] <= kth[r])  # ascending index: a stable sort on d2 keeps ties in index order
        o = cand[np.argsort(dd[r, cand], kind="stable")[:km1]]
        idx[r], d2[r] = o, dd[r, o]
    return idx, d2


def knn(x, n_neighbors, block=128, threads=None):
    """(knn_indices int32, knn_distances float32, knn_d2 float64), each n x (k - 1), rule 3 order.  Row blocks run on
    a thread pool (they are independent; numpy releases the GIL)."""
    x = np.asarray(x, dtype=np.float32)
    n, km1 = x.shape[0], n_neighbors - 1
    blocks = [np.arange(r0, min(n, r0 + block)) for r0 in range(0, n, block)]
    threads = threads or min(16, os.cpu_count() or 1, len(blocks))
    if threads > 1:
        with ThreadPoolExecutor(threads) as ex:
            res = list(ex.map(lambda rows: _knn_block(x, rows, km1), blocks))
    else:
        res = [_knn_block(x, rows, km1) for rows in blocks]
    idx = np.concatenate([r[0] for r in res])
    d2 = np.concatenate([r[1] for r in res])
    return idx, np.sqrt(d2).astype(np.float32), d2


def _seq_sum(a):
    """Row sums in column order (np.sum is pairwise)."""
    s = np.zeros(a.shape[0], dtype=np.float64)
    for j in range(a.shape[1]):
        s = s + a[:, j]
    return s


def smooth(knn_dist, n_neighbors):
    """(rho, sigma, weights, floored): float64; floored marks the rows whose sigma is the floor."""
    delta = np.asarray(knn_dist, dtype=np.float32).astype(np.float64)
    n, km1 = delta.shape
    assert km1 == n_neighbors - 1
    target = np.log2(float(n_neighbors))
    pos = delta > 0
    rho = np.where(pos.any(axis=1), np.where(pos, delta, np.inf).min(axis=1), 0.0)
    g = np.maximum(delta - rho[:, None], 0.0)
    lo = np.zeros(n)
    hi = np.full(n, np.inf)
    mid = np.ones(n)
    active = np.ones(n, dtype=bool)
    for _ in range(64):
        s = _seq_sum(np.exp(-(g / mid[:, None])))
        active &= ~(np.abs(s - target) < 1e-5)
        if not active.any():
            break
        up = active & (s > target)
        dn = active & ~(s > target)
        hi = np.where(up, mid, hi)
        lo = np.where(dn, mid, lo)
        with np.errstate(invalid="ignore", over="ignore"):
            new = np.where(up, (lo + hi) / 2.0, np.where(np.isinf(hi), mid * 2.0, (lo + hi) / 2.0))
        mid = np.where(active, new, mid)
    row_mean = _seq_sum(delta) / km1
    # the global mean's summation order is the only order-dependent sum: rows in order, each row's sum first
    total = 0.0
    for v in _seq_sum(delta):
        total += v
    floor = np.where(rho > 0, 1e-3 * row_mean, 1e-3 * (total / (float(n) * float(km1))))
    floored = mid < floor
    sigma = np.where(floored, floor, mid)
    gg = delta - rho[:, None]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        w = np.where(gg <= 0, 1.0, np.exp(-(gg / sigma[:, None])))
    return rho, sigma, w, floored


def distances_csr(knn_idx, knn_dist):
    n, km1 = knn_idx.shape
    order = np.argsort(knn_idx, axis=1, kind="stable")
    cols = np.take_along_axis(knn_idx, order, axis=1).astype(np.int32)
    vals = np.take_along_axis(knn_dist, order, axis=1).astype(np.float32)
    return sp.csr_matrix((vals.ravel(), cols.ravel(), np.arange(n + 1, dtype=np.int64) * km1), shape=(n, n))


def connectivities_csr(knn_idx, w):
    n, km1 = knn_idx.shape
    a = sp.csr_matrix((w.ravel(), knn_idx.ravel().astype(np.int64), np.arange(n + 1, dtype=np.int64) * km1),
                      shape=(n, n))
    at = a.T.tocsr()
    c = (a + at - a.multiply(at)).tocsr().astype(np.float32)
    c.eliminate_zeros()
    c.sort_indices()
    return c


def neighbors(x, n_neighbors):
    """dict with knn_indices, knn_distances, rho, sigma, floored, distances, connectivities."""
    idx, dist, _ = knn(x, n_neighbors)
    rho, sigma, w, floored = smooth(dist, n_neighbors)
    return {"knn_indices": idx, "knn_distances": dist, "rho": rho, "sigma": sigma, "floored": floored, "weights": w,
            "distances": distances_csr(idx, dist), "connectivities": connectivities_csr(idx, w)}


# ---- test inputs ------------------------------------------------------------------------------------------------------
def mixture(n, d, seed=0, offset=0.0, n_clusters=6):
    """Gaussian mixture with an anisotropic spread like PCA scores (column c scaled by ~ 1 / sqrt(c + 1)); every
    column is shifted by `offset` times the standard deviation of the widest one."""
    rng = np.random.default_rng(seed)
    scale = 3.0 / np.sqrt(np.arange(d) + 1.0)
    centres = rng.normal(size=(n_clusters, d)) * scale * 2.0
    lab = rng.integers(0, n_clusters, size=n)
    x = centres[lab] + rng.normal(size=(n, d)) * scale
    return (x + offset * x[:, 0].std()).astype(np.float32)


def hub(n=3000, d=50, seed=0):
    """Normal points normalised to radius 5 and cell 0 at the origin: in 50 dimensions the others are ~ 7 apart, so
    cell 0 is every cell's nearest neighbour and its connectivity row has n - 1 entries."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d))
    x *= 5.0 / np.sqrt((x * x).sum(axis=1, keepdims=True))
    x[0] = 0.0
    return x.astype(np.float32)


def small_clusters(n_clusters=60, size=10, d=5, spread=1e6, seed=0):
    """Unit-normal clusters of `size` cells (fewer than k) with centres `spread` apart: a row's k - 1 neighbours are
    its size - 1 cluster mates and then very far cells, whose membership strengths are 0 in float32."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(n_clusters, d)) * spread
    return (np.repeat(centres, size, axis=0) + rng.normal(size=(n_clusters * size, d))).astype(np.float32)


def simplex(n=64):
    """The n unit vectors: every d2 is 2, so every neighbour is a tie that goes to the lower index."""
    return np.eye(n, dtype=np.float32)


def near_duplicates():
    """The 3000 x 50 mixture with the duplicate blocks of test_duplicate_blocks, rows 2001 .. 2069 set to row 2000 moved
    by a few float32 ulps in ONE column each, up (odd row) or down (even row).  Columns are taken by ascending magnitude
    of row 2000.  Row 2000 holds one value below 2^-5 and two more below 2^-3, so one-ulp steps alone give only three
    distinct distances up to 1.49e-8; rows 2001 .. 2010 therefore step 1, 1, 2, 2, ... 5, 5 ulps in the smallest column
    (2^-29 each), and rows 2011 .. 2069 step one ulp in the following columns, two rows per column.  The 14 nearest
    neighbours of row 2000 are then at 1, 2, 3, 4, 5 x 2^-29 with 4 x 2^-29 = 2^-27 a tie between a four-ulp step and
    the one-ulp steps of the next two columns: d2 ~ 1e-17 against float32 keys of order 1."""
    x = mixture(3000, 50, seed=11)
    x[100:111] = x[100]
    x[[5, 900, 2999]] = x[5]
    x[2000:2070] = x[2000]
    order = np.argsort(np.abs(x[2000]), kind="stable")
    for m in range(1, 70):
        c, steps = (order[0], (m + 1) // 2) if m <= 10 else (order[(m - 9) // 2], 1)
        for _ in range(steps):
            x[2000 + m, c] = np.nextafter(x[2000 + m, c], np.float32(np.inf if m % 2 else -np.inf))
    return x


LADDER_K = 30


def ladder(m=12, n_far=30, d=3, lo=75.0, hi=145.0, seed=0):
    """A unit-normal cluster of m cells and n_far cells on the first axis at lo .. hi in equal steps, for
    k = LADDER_K = 30.  A cluster row (sigma ~ 1) lists its m - 1 mates and the k - m nearest rungs with strengths
    exp(-75 / sigma) .. exp(-116 / sigma): through the float32 subnormals down to 0.  The rungs are nearer to one another than
    to the cluster and list only rungs, so those strengths reach the connectivities unsymmetrised."""
    rng = np.random.default_rng(seed)
    far = np.zeros((n_far, d))
    far[:, 0] = np.linspace(lo, hi, n_far)
    return np.concatenate([rng.normal(size=(m, d)), far]).astype(np.float32)


def scaled(x, p):
    """x times 2^p in float32: exact while nothing overflows or becomes subnormal."""
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(x, dtype=np.float32) * np.float32(2.0**p)

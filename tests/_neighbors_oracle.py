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

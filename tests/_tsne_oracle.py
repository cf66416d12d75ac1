"""numpy oracle of tl.tsne: DESIGN.md 4.12 restated (the specification).

sklearn's sparse affinities and the EXACT repulsion over all n (n - 1) ordered pairs, optimised with the rules of
sklearn's ``_gradient_descent``, as a pure function of (X_rep, parameters, random_state, initial positions).

1. Neighbours: the kk = min(floor(3 perplexity), 63, n - 1) exact nearest neighbours of every row (pp.neighbors' rules);
   perplexity >= kk is an error.
2. Conditional affinities, float64, one row at a time: rel_r = d_r d_r - d_0 d_0 of the stored float32 distances;
   e_r = EXP(-(beta rel_r)), S = sum e_r, E = sum rel_r e_r (both in neighbour order); the entropy is above its target
   log(perplexity) iff S > EXP(log(perplexity) - (beta E) / S).  beta = 1 is doubled (entropy above) or halved until
   both sides have been seen (at most 64 evaluations, else the last beta stands); then 64 times beta = (lo + hi) / 2 is
   evaluated and replaces lo (entropy above) or hi; the result is (lo + hi) / 2.  p_r = e_r / S.  A row whose
   distances are all equal has beta = 1 and p = 1 / kk.  EXP is the WRITTEN exponential :func:`exp_` (IEEE operations
   in a fixed order), so beta and p have one value on every machine.
3. W = A + A^T in float64 (A holds p at the neighbour columns), stored as float32 canonical CSR without zeros;
   P = W / (2 n), and the factor stays in the gradient.
4. Repulsion, float32, every operation rounded, all j != i: dx_c = y_ic - y_jc, d2 = dx_0^2 + dx_1^2 (+ dx_2^2),
   q = 1 / (1 + d2) correctly rounded, Zr_i = sum_j rint(q 2^32), R_ic = sum_j rint(((q q) dx_c) 2^32): int64 sums.
   H = sum_i (Zr_i >> 32), L = sum_i (Zr_i & 0xffffffff), Z = double(H) + double(L) 2^-32.
5. Attraction, float64, the stored entries e = (i, j) of row i: d = double(y_i) - double(y_j), d2 left to right,
   q = 1 / (1 + d2), A_ic = sum_e rint(((double(W_e) q) d_c) 2^40): an int64 sum.
6. g_ic = 4 ((ex_t / (2 n)) (double(A_ic) 2^-40) - (double(R_ic) 2^-32) / Z)  (the second term is 0 when Z = 0: n = 1);
   with u, gain, y the float32 state read as float64: gain' = float32(max(u g < 0 ? gain + 0.2 : gain 0.8, 0.01)),
   u' = float32(m_t u - eta (double(gain') g)), y' = float32(y + double(u')).  ex_t = early_exaggeration and
   m_t = 0.5 for t < exaggeration_iters (250), else 1 and 0.8.  No early stopping.
7. Initial positions: "pca" = the first c columns of the representation / std(column 0) * 1e-4 in float64, stored as
   float32; "random" = counter hash (tag 2^64 - 3), uniform with standard deviation 1e-4.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp

import _umap_oracle as uo

TAG_TSNE = uo.MASK - 2
MAX_NEIGHBORS = 63
LONG_ROW = 512  # rows above this many entries take a workgroup on the device (nothing changes in the numbers)

_LOG2E = 1.4426950408889634
_LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
_LN2_LO = 1.9082149292705877e-10
_EXP_C = (1.6059043836821613e-10, 2.08767569878681e-09, 2.505210838544172e-08, 2.755731922398589e-07,
          2.7557319223985893e-06, 2.48015873015873e-05, 0.0001984126984126984, 0.001388888888888889,
          0.008333333333333333, 0.041666666666666664, 0.16666666666666666, 0.5)  # 1 / 13! .. 1 / 2!


def exp_(x):
    """The written exponential of rule 2: 0 below -708 (and for NaN), else with k = rint(x log2 e) and
    r = (x - k ln2_hi) - k ln2_lo the Taylor polynomial of degree 13 in Horner form, times 2^k."""
    x = np.asarray(x, dtype=np.float64)
    ok = x >= -708.0
    xs = np.where(ok, x, 0.0)
    k = np.rint(xs * _LOG2E)
    r = (xs - k * _LN2_HI) - k * _LN2_LO
    p = np.full_like(r, _EXP_C[0])
    for c in _EXP_C[1:]:
        p = p * r + c
    p = p * r + 1.0
    p = p * r + 1.0
    return np.where(ok, np.ldexp(p, k.astype(np.int64)), 0.0)


def n_neighbors(n, perplexity):
    return min(int(math.floor(3.0 * perplexity)), MAX_NEIGHBORS, n - 1)


def _seq_sum(a):
    s = np.zeros(a.shape[0], dtype=np.float64)
    for j in range(a.shape[1]):
        s = s + a[:, j]
    return s


def _above(rel, beta, target):
    e = exp_(-(beta[:, None] * rel))
    S = _seq_sum(e)
    E = _seq_sum(rel * e)
    return S > exp_(target - (beta * E) / S)


def affinities(knn_dist, perplexity):
    """(beta n, p n x kk) of rule 2 for the float32 distances (nearest first)."""
    d = np.asarray(knn_dist, dtype=np.float32).astype(np.float64)
    n, kk = d.shape
    d2 = d * d
    rel = d2 - d2[:, :1]
    target = math.log(float(perplexity))
    flat = rel[:, -1] == 0.0
    lo = np.zeros(n)
    hi = np.full(n, np.inf)
    beta = np.ones(n)
    searching = ~flat
    for step in range(64):
        if not searching.any():
            break
        up = _above(rel, beta, target)
        lo = np.where(searching & up, beta, lo)
        hi = np.where(searching & ~up, beta, hi)
        searching &= ~((lo > 0.0) & (hi < np.inf))
        if step < 63:
            beta = np.where(searching, np.where(up, beta * 2.0, beta / 2.0), beta)
    found = (lo > 0.0) & (hi < np.inf)
    for _ in range(64):
        mid = np.where(found, (lo + hi) / 2.0, beta)
        up = _above(rel, mid, target)
        lo = np.where(found & up, mid, lo)
        hi = np.where(found & ~up, mid, hi)
    beta = np.where(found, (lo + hi) / 2.0, beta)
    e = exp_(-(beta[:, None] * rel))
    p = e / _seq_sum(e)[:, None]
    p[flat] = 1.0 / kk
    return beta, p


def symmetrize(knn_idx, p):
    """W of rule 3 (float32 canonical CSR)."""
    n, kk = knn_idx.shape
    a = sp.csr_matrix((p.ravel(), knn_idx.ravel().astype(np.int64), np.arange(n + 1, dtype=np.int64) * kk), shape=(n, n))
    w = (a + a.T.tocsr()).tocsr().astype(np.float32)
    w.eliminate_zeros()
    w.sort_indices()
    return w


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


def _q32(v):
    return np.rint(v.astype(np.float64) * 4294967296.0).astype(np.int64)


def repulsion(y, block=512, return_abs=False):
    """(Zr int64 n, R int64 n x c) of rule 4; with return_abs also sum_j |q q dx_c| (float64, for error bounds)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    n, c = y.shape
    Zr = np.zeros(n, dtype=np.int64)
    R = np.zeros((n, c), dtype=np.int64)
    absum = np.zeros((n, c))
    one = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for r0 in range(0, n, block):
            rows = np.arange(r0, min(n, r0 + block))
            dx = [y[rows, q, None] - y[None, :, q] for q in range(c)]
            d2 = dx[0] * dx[0] + dx[1] * dx[1]
            if c == 3:
                d2 = d2 + dx[2] * dx[2]
            q = one / (one + d2)
            assert q.dtype == np.float32
            zq = _q32(q)
            zq[np.arange(len(rows)), rows] = 0  # the pair (i, i), by index
            Zr[rows] = zq.sum(axis=1)
            qq = q * q
            for k in range(c):
                t = qq * dx[k]
                assert t.dtype == np.float32
                tq = _q32(t)
                tq[np.arange(len(rows)), rows] = 0
                R[rows, k] = tq.sum(axis=1)
                if return_abs:
                    absum[rows, k] = np.abs(t.astype(np.float64)).sum(axis=1)
    return (Zr, R, absum) if return_abs else (Zr, R)


def normaliser(Zr):
    H = int((Zr >> 32).sum())
    L = int((Zr & 0xFFFFFFFF).sum())
    return float(H) + float(L) * 2.0 ** -32


def attraction(g, y, return_abs=False):
    """A int64 n x c of rule 5."""
    y64 = np.asarray(y, dtype=np.float32).astype(np.float64)
    c = y64.shape[1]
    d = y64[g.rows] - y64[g.indices]
    d2 = d[:, 0] * d[:, 0]
    for k in range(1, c):
        d2 = d2 + d[:, k] * d[:, k]
    q = 1.0 / (1.0 + d2)
    t = (g.w * q)[:, None] * d
    A = np.zeros((g.n, c), dtype=np.int64)
    np.add.at(A, g.rows, np.rint(t * 2.0 ** 40).astype(np.int64))
    if return_abs:
        ab = np.zeros((g.n, c))
        np.add.at(ab, g.rows, np.abs(t))
        return A, ab
    return A


def schedule(t, early_exaggeration=12.0, exaggeration_iters=250):
    """(ex_t, m_t)"""
    return (float(early_exaggeration), 0.5) if t < exaggeration_iters else (1.0, 0.8)


def gradient(g, y, ex):
    """g of rule 6 (float64 n x c)."""
    Zr, R = repulsion(y)
    Z = normaliser(Zr)
    A = attraction(g, y)
    rep = (R.astype(np.float64) * 2.0 ** -32) / Z if Z > 0 else np.zeros(R.shape)
    return 4.0 * ((ex / (2.0 * g.n)) * (A.astype(np.float64) * 2.0 ** -40) - rep)


def iteration(g, y, u, gain, t, *, early_exaggeration=12.0, exaggeration_iters=250, learning_rate=1000.0, grad=None):
    """One iteration of rule 6 on the float32 state; returns the new (y, u, gain)."""
    ex, m = schedule(t, early_exaggeration, exaggeration_iters)
    gr = gradient(g, y, ex) if grad is None else grad
    y64, u64, g64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (y, u, gain))
    with np.errstate(over="ignore", invalid="ignore"):
        inc = u64 * gr < 0.0
        gn = np.maximum(np.where(inc, g64 + 0.2, g64 * 0.8), 0.01).astype(np.float32)
        un = (m * u64 - float(learning_rate) * (gn.astype(np.float64) * gr)).astype(np.float32)
        yn = (y64 + un.astype(np.float64)).astype(np.float32)
    return yn, un, gn


def start(y0):
    y0 = np.ascontiguousarray(y0, dtype=np.float32)
    return y0, np.zeros_like(y0), np.ones_like(y0)


def run(g, state, t0, t1, keep=(), **kw):
    """The iterations [t0, t1) on state = (y, u, gain); `keep`: iterations whose state BEFORE them is returned too."""
    snaps = {}
    for t in range(t0, t1):
        if t in keep:
            snaps[t] = state
        state = iteration(g, *state, t, **kw)
    return (state, snaps) if keep else state


def random_init(n, c, seed):
    """init_pos="random": uniform on [-sqrt(3), sqrt(3)) 1e-4 (standard deviation 1e-4)."""
    return ((uo.uniform24(seed, TAG_TSNE, n, c) * 2.0 - 1.0) * (math.sqrt(3.0) * 1e-4)).astype(np.float32)


def pca_init(x, c):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return (x[:, :c] / np.std(x[:, 0]) * 1e-4).astype(np.float32)


def tsne(x, *, perplexity=30.0, n_components=2, max_iter=1000, init_pos="pca", random_state=0, early_exaggeration=12.0,
         learning_rate=1000.0):
    """The whole contract on the host: (y, info)."""
    import _neighbors_oracle as no

    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    kk = n_neighbors(n, perplexity)
    if perplexity >= kk:
        raise ValueError("perplexity")
    idx, dist, _ = no.knn(x, kk + 1)
    beta, p = affinities(dist, perplexity)
    w = symmetrize(idx, p)
    y0 = pca_init(x, n_components) if init_pos == "pca" else random_init(n, n_components, random_state)
    state = run(Graph(w), start(y0), 0, max_iter, early_exaggeration=early_exaggeration, learning_rate=learning_rate)
    return state[0], {"knn_indices": idx, "knn_distances": dist, "beta": beta, "cond": p, "W": w}

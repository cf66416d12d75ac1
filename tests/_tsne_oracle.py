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
TILE = 256  # positions per LDS tile of the device's repulsion (nothing changes in the numbers)

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


def repulsion_grouped(y):
    """:func:`repulsion` for positions that take few distinct values: the m x m quantised terms of the distinct points
    once, times the number of cells at each point (int64), minus rint(2^32) for the pair (i, i) (its R term is 0), and
    scattered back to the cells.  The sums are integer sums, so the result equals ``repulsion(y)`` exactly."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    pts, inv, cnt = np.unique(y, axis=0, return_inverse=True, return_counts=True)
    inv, cnt = np.asarray(inv).reshape(-1), cnt.astype(np.int64)
    c = y.shape[1]
    one = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dx = [pts[:, k, None] - pts[None, :, k] for k in range(c)]
        d2 = dx[0] * dx[0] + dx[1] * dx[1]
        if c == 3:
            d2 = d2 + dx[2] * dx[2]
        q = one / (one + d2)
        qq = q * q
        assert qq.dtype == np.float32
        Zr = _q32(q) @ cnt - (1 << 32)
        R = np.stack([_q32(qq * dx[k]) @ cnt for k in range(c)], axis=1)
    return Zr[inv], R[inv]


def gradient(g, y, ex, repulse=repulsion):
    """g of rule 6 (float64 n x c); `repulse`: :func:`repulsion` or :func:`repulsion_grouped`."""
    Zr, R = repulse(y)
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


# ---- the device's geometry and the inputs of the edge tests (tests/test_gpu_tsne_edges.py; test_tsne_oracle.py asserts
# ---- on the CPU that each of them enters the branch it is for) -----------------------------------------------------------
def repulse_geometry(n):
    """(i_blocks, tiles, split, chunk, grid_y) of the device's repulsion grid: icv_tsne_iterations' integer arithmetic.
    A workgroup (bx, by) owns the cells [256 bx, +256) and streams the positions [chunk by, +chunk) in tiles of TILE."""
    i_blocks = (n + 255) // 256
    split = (2048 + i_blocks - 1) // i_blocks
    tiles = (n + TILE - 1) // TILE
    split = min(max(1, min(split, tiles)), 65535)
    chunk = (tiles + split - 1) // split * TILE
    return i_blocks, tiles, split, chunk, (n + chunk - 1) // chunk


def affinities_steps(knn_dist, perplexity):
    """The evaluation of the doubling / halving phase of rule 2 at which each row has seen both sides: 0 .. 63, -1 for a
    row that never does (beta stays 2^63 or 2^-63), -2 for a row of equal distances."""
    d = np.asarray(knn_dist, dtype=np.float32).astype(np.float64)
    rel = d * d - (d * d)[:, :1]
    target = math.log(float(perplexity))
    n = len(d)
    steps = np.where(rel[:, -1] == 0.0, -2, -1)
    seen_up, seen_down, beta = np.zeros(n, bool), np.zeros(n, bool), np.ones(n)
    for step in range(64):
        up = _above(rel, beta, target)
        seen_up |= up
        seen_down |= ~up
        steps = np.where((steps == -1) & seen_up & seen_down, step, steps)
        beta = np.where(up, beta * 2.0, beta / 2.0)
    return steps


TILE_SIZES = (11520, 11521, 16385)  # chunk 256 (the largest such n) / 512 / 768, the last two with a 257-cell last chunk
TILE_VARIANTS = ("drawn", "lonely_last", "second_tile")


def tile_positions(n, c, variant, seed=0):
    """n cells drawn from 100 distinct float32 points, so that every tile holds other counts and the grouped oracle
    applies.  "lonely_last": cell n - 1 alone at a point of its own (dropping the last tile changes Z); "second_tile":
    the cells 256 .. 511 sit on cell 0."""
    rng = np.random.default_rng([seed, n, c])
    pts = rng.normal(size=(101, c)).astype(np.float32)
    y = pts[rng.integers(0, 100, n)]
    if variant == "lonely_last":
        y[n - 1] = pts[100]
    elif variant == "second_tile":
        y[TILE:2 * TILE] = y[0]
    else:
        assert variant == "drawn"
    return np.ascontiguousarray(y)


def ring_graph(n, offsets=(1, 7, 300, 5000), seed=0):
    """Symmetric, 2 len(offsets) entries per row: i -- (i + o) mod n with seeded float32 weights in (0, 2]."""
    rng = np.random.default_rng([seed, n])
    i = np.arange(n, dtype=np.int64)
    rows = np.concatenate([i for _ in offsets])
    cols = np.concatenate([(i + o) % n for o in offsets])
    w = (np.float32(2.0) * (np.float32(1.0) - rng.random(len(rows), dtype=np.float32))).astype(np.float64)
    g = sp.coo_matrix((np.r_[w, w], (np.r_[rows, cols], np.r_[cols, rows])), shape=(n, n)).tocsr()
    g.sort_indices()
    assert g.nnz == 2 * len(rows) and g.data.max() <= 2.0 and g.data.min() > 0.0
    return g


GAINS = (0.01, 0.012, 0.0125, 1.0, 1e3)  # 0.8 times the first two is below the floor, 0.8 times the third is at it
UPDATES = (0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 1e6, -1e6)


def crafted_state(y, scale=None):
    """(y, u, gain) with every pair of GAINS x UPDATES (coordinate k takes GAINS[k mod 5] and UPDATES[k mod 8]);
    `scale` multiplies the updates (the tile tests use small ones so that the positions stay where they are)."""
    y = np.ascontiguousarray(y, dtype=np.float32)
    k = np.arange(y.size)
    u = np.asarray(UPDATES, dtype=np.float32)[k % 8].reshape(y.shape)
    if scale is not None:
        u = u * np.float32(scale)
    return y, u, np.asarray(GAINS, dtype=np.float32)[k % 5].reshape(y.shape)


ROW_GRAPHS = {"star511": 0, "star512": 0, "star513": 1, "star768": 1, "two_centres": 2, "last_vertex": 1}  # long rows


def row_graph(name, seed=0):
    """Graphs whose longest rows sit at LONG_ROW: stars with a centre row of 511 / 512 / 513 / 768 entries, two centres
    of 513 and 600 entries, and a 600-entry row that is the last vertex.  One stored weight is exactly 2, one a
    float32 subnormal and one a stored 0 (all three in a centre row and in a leaf's)."""
    if name.startswith("star"):
        m = int(name[4:])
        rows, cols, n = np.zeros(m, dtype=np.int64), np.arange(1, m + 1), m + 1
    elif name == "two_centres":  # row 0: 1 .. 513; row 1: 0 and 2 .. 600
        rows = np.r_[np.zeros(513, dtype=np.int64), np.ones(599, dtype=np.int64)]
        cols, n = np.r_[np.arange(1, 514), np.arange(2, 601)], 601
    else:
        assert name == "last_vertex"
        rows, cols, n = np.full(600, 600, dtype=np.int64), np.arange(600), 601
    rng = np.random.default_rng([seed, len(rows)])
    w = rng.random(len(rows)) + 0.01
    w = (w * (2.0 / w.max())).astype(np.float32)
    pick = rng.choice(np.flatnonzero(w < 2.0), 2, replace=False)
    w[pick[0]], w[pick[1]] = np.float32(1e-40), 0.0
    w = w.astype(np.float64)
    g = sp.coo_matrix((np.r_[w, w], (np.r_[rows, cols], np.r_[cols, rows])), shape=(n, n)).tocsr()
    g.sort_indices()
    return g


AFFINITY_KK = (1, 2, 15, 63)
AFFINITY_N = (1, 255, 256, 257, 1000)
AFFINITY_EXPONENTS = tuple(range(-62, 63, 4))
AFFINITY_KINDS = ("scaled", "flat", "d0_positive", "scaled", "nine_zeros", "underflow")


def affinity_base(kk):
    """Sorted, d_0 = 0: rel_r = r / 4.  At kk = 15 beta is 2.1965 (perplexity 5) and 0.010691 (perplexity 14.999)."""
    return (np.sqrt(np.arange(kk)) * 0.5).astype(np.float32)


def affinity_scaled(kk):
    """(rows, e): the base row times 2^e for every e of AFFINITY_EXPONENTS (exact in float32 and in every product of
    rule 2, so beta shifts by exactly 2^-2e while the doubling / halving brackets it)."""
    e = np.asarray(AFFINITY_EXPONENTS)
    return np.ldexp(affinity_base(kk)[None, :], e[:, None]).astype(np.float32), e


def affinity_perplexities(kk):
    return tuple(p for p in (5.0, kk - 1e-3) if p < kk)


def affinity_rows(kk, n):
    """(distances n x kk float32, kind of each row): the kinds of AFFINITY_KINDS interleaved so that every wavefront
    holds all of them; the scaled rows alternate between the two ends of AFFINITY_EXPONENTS and walk inwards."""
    scaled, _ = affinity_scaled(kk)
    m = len(scaled)
    order = [j // 2 if j % 2 == 0 else m - 1 - j // 2 for j in range(m)]
    base = affinity_base(kk)
    d = np.zeros((n, kk), dtype=np.float32)
    kinds = []
    s = 0
    for r in range(n):
        kind = AFFINITY_KINDS[r % len(AFFINITY_KINDS)]
        kinds.append(kind)
        if kind == "scaled":
            d[r] = scaled[order[s % m]]
            s += 1
        elif kind == "flat":  # 0, 3, 1e-30 (the square underflows in float32, not in float64), 1e30
            d[r] = (0.0, 3.0, 1e-30, 1e30)[(r // 6) % 4]
        elif kind == "d0_positive":
            d[r] = np.float32(0.75) + base * np.float32(1 + (r // 6) % 5)
        elif kind == "nine_zeros":
            d[r, 9:] = base[:max(kk - 9, 0)] + np.float32(0.25)
        else:  # up to 7 neighbours near 1, the others from 40 on: beta (rel_r) > 708 for them at perplexity 5
            d[r] = np.float32(1.0) + base * np.float32(0.125)
            d[r, 7:] = np.float32(40.0) + base[:max(kk - 7, 0)]
            d[r, 0] = 0.0
    assert (np.diff(d, axis=1) >= 0).all()
    return d, np.asarray(kinds)


UPDATE_CASES = ("crossed", "zero_gradient", "far_line", "huge")


def update_case(name, c, n=300, seed=0):
    """(graph, state, what the CPU test asserts about it) for rule 6:
    "crossed": GAINS x UPDATES x both signs of the gradient on a ring graph, positions N(0, 1);
    "zero_gradient": no stored entry and coincident positions: g = 0 exactly while u != 0;
    "far_line": cells 1e6 apart on a line: every q < 2^-33, so Z = 0 with n > 1;
    "huge": positions 2^19 N(0, 1): d2 reaches 1e11 and most terms quantise to 0 or +-1."""
    rng = np.random.default_rng([seed, c, n])
    g = ring_graph(n, offsets=(1, 7, 30), seed=seed)
    if name == "crossed":
        y = rng.normal(size=(n, c)).astype(np.float32)
    elif name == "zero_gradient":
        g = sp.csr_matrix((n, n), dtype=np.float64)
        y = np.zeros((n, c), dtype=np.float32) + rng.normal(size=c).astype(np.float32)
    elif name == "far_line":
        y = np.zeros((n, c), dtype=np.float32)
        y[:, 0] = np.arange(n) * 1e6
    else:
        assert name == "huge"
        y = (rng.normal(size=(n, c)) * 2.0 ** 19).astype(np.float32)
    return g, crafted_state(y)

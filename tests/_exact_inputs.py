"""Inputs on which the float32 Gram kernels make no rounding error, and their exact answers.

The fp32 MFMA Gram (``k_gram_mfma``) serves the cell-cell correlations of ``tl.ithcna`` / ``tl.ithgex`` and the
squared distances of ``tl.cell_linkage``.  Compared with float64 numpy it can only be held to a tolerance, and a
tolerance hides what a selection or tiling kernel gets wrong (a rank off by one, a lost K stage).  On the inputs
built here every float32 operation of those kernels is exact, so the GPU result must equal the reference bit for bit.

Correlations.  Each pattern is a length-k row with exactly N = 4^j nonzero entries, half +1 and half -1.  Cell i
is ``pattern[label_i] * 2^e_i + c_i``: its float64 mean (``k_row_normalize``) is exactly ``c_i``, the norm of the
centred row is ``2^(j + e_i)``, so z has entries 0 and +-2^-j, and every partial sum of a z.z dot product is a
multiple of 1/N no larger than 1 in magnitude.  The correlation matrix is exactly ``P[l] P[l]^T / N``.

Distances.  Integer rows A in [-7, 7] and their negatives (plus a zero row for odd n), shuffled, with an integer
offset per column: the float64 column mean is the offset, the centred values are small integers, and every partial
Gram sum is an integer below 2^24.  The squared distances are exact in int64.
"""
from __future__ import annotations

import numpy as np


# --------------------------------------------------------------------------------------------------------------- #
# correlations
# --------------------------------------------------------------------------------------------------------------- #
def support_size(k):
    """The largest N = 4^j <= k (N = 4 for k < 16, so a 4-column row still has a nonzero pattern)."""
    assert k >= 4
    n = 4
    while n * 4 <= k:
        n *= 4
    return n


def corr_patterns(p, k, N, rng, cols=None):
    """p int8 patterns of length k: N entries +-1 (half each) in random columns (of ``cols``, default all)."""
    assert N >= 4 and N & (N - 1) == 0 and (N.bit_length() - 1) % 2 == 0, "N must be a power of 4"
    cols = np.arange(k) if cols is None else np.asarray(cols)
    assert N <= len(cols)
    P = np.zeros((p, k), dtype=np.int8)
    for a in range(p):
        where = rng.choice(cols, N, replace=False)
        P[a, where[: N // 2]] = 1
        P[a, where[N // 2:]] = -1
    return P


def corr_cells(P, labels, rng, exps=(-2, -1, 0, 1, 2), offsets=range(-8, 9), scale=True, offset=True):
    """float32 cells ``P[labels] * 2^e + c`` (per-row exponent e and integer offset c)."""
    labels = np.asarray(labels)
    n = len(labels)
    e = rng.choice(np.asarray(exps), n) if scale else np.zeros(n, dtype=np.int64)
    c = rng.choice(np.asarray(list(offsets)), n) if offset else np.zeros(n, dtype=np.int64)
    X = P[labels].astype(np.float64) * np.ldexp(1.0, e)[:, None] + c[:, None]
    X32 = X.astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), X)
    return X32


def exact_corr(P, labels, N):
    """The exact correlation matrix of the cells of ``corr_cells`` (float64; every entry a multiple of 1/N)."""
    Q = P[np.asarray(labels)].astype(np.float64)
    return (Q @ Q.T) / N


def corr_case(n, k, p, seed, N=None, **kw):
    """(X float32 n x k, labels, P, N): n cells drawn from p patterns (every pattern used when n >= p)."""
    rng = np.random.default_rng(seed)
    N = support_size(k) if N is None else N
    P = corr_patterns(p, k, N, rng)
    labels = np.concatenate([np.arange(min(p, n)), rng.integers(0, p, max(n - p, 0))])
    rng.shuffle(labels)
    return corr_cells(P, labels, rng, **kw), labels, P, N


def lerp(a, b, t):
    """numpy's ``_lerp`` rule for one value (what ``np.percentile(..., method="linear")`` does)."""
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def weighted_percentile(values, weights, qs, shift=0):
    """``np.percentile`` of the multiset holding ``values[i]`` ``weights[i]`` times (integer weights), without
    materialising it: the ranks floor(q (m - 1)) and the next one from the cumulative weights, then ``lerp``.
    ``shift``: both ranks moved by that much (what a selection with an off-by-one would return)."""
    values = np.asarray(values, dtype=np.float64).ravel()
    weights = np.asarray(weights, dtype=np.int64).ravel()
    order = np.argsort(values, kind="stable")
    v, cum = values[order], np.cumsum(weights[order])
    m = int(cum[-1])
    out = []
    for q in qs:
        pos = (m - 1) * (q / 100.0)
        r = min(max(int(np.floor(pos)) + shift, 0), m - 1)
        r1 = min(r + 1, m - 1)
        a = v[np.searchsorted(cum, r, side="right")]
        b = v[np.searchsorted(cum, r1, side="right")]
        out.append(lerp(a, b, pos - np.floor(pos)))  # the weight of the unshifted position
    return out


def pattern_iqr(P, N, counts, shift=0):
    """IQR of the correlation matrix of a group with ``counts[a]`` cells of pattern a (any scales and offsets):
    the entries are ``corr(a, b)`` with weight ``counts[a] * counts[b]``."""
    Pf = P.astype(np.float64)
    V = (Pf @ Pf.T) / N
    c = np.asarray(counts, dtype=np.int64)
    q75, q25 = weighted_percentile(V, np.outer(c, c), [75, 25], shift)
    return q75 - q25


def rank_boundary_case(n, k, seed, N=None):
    """(X, labels, P, N, counts) of a group of n = 4j cells whose IQR changes when the percentile ranks move by one.

    Heavy ties make a large group blind to an off-by-one unless a rank sits on the edge of a run of equal values.
    Patterns 0 and 1 are opposite (correlation -1, the smallest entry) and pattern 2 is neither; with j, 2j and j
    cells the value -1 fills exactly 2 * j * 2j = n^2 / 4 entries, the ranks 0 .. floor(0.25 (n^2 - 1)), so q25
    interpolates between the last -1 and the next value."""
    assert n % 4 == 0
    rng = np.random.default_rng(seed)
    N = support_size(k) if N is None else N
    while True:
        P = corr_patterns(3, k, N, rng)
        P[1] = -P[0]
        V = P.astype(np.int64) @ P.T.astype(np.int64)
        if V[0, 2] > -N and V[1, 2] > -N:
            break
    j = n // 4
    counts = np.array([j, 2 * j, j])
    labels = rng.permutation(np.repeat(np.arange(3), counts))
    return corr_cells(P, labels, rng), labels, P, N, counts


def iqr(C):
    """The reference's score: ``q75 - q25`` of ``np.percentile`` over all entries."""
    q75, q25 = np.percentile(C, [75, 25])
    return q75 - q25


def tie_break_case():
    """(X float32 8 x 81, exact correlation matrix): a group whose IQR changes when either percentile rank moves by
    one AND when numpy's two ``_lerp`` branches are swapped.

    Cell 0 carries two extra entries +-2^-51 in columns no other cell uses except cell 1, which has +1/8 (one of its
    64 entries +-1/8) in column ``p``.  Cell 0's mean is exactly 0 and its squared norm rounds to exactly 4 in
    float64, so its z is exact: +-1/2 and +-2^-52.  corr(0, 1) is then the single product 2^-52 / 8 = 2^-55 (the
    two cells share no other column).  Sorted, the 64 entries are 46 zeros, 2^-55 twice, 0.5 four times and 1
    twelve times: q75 interpolates at t = 0.25 between 2^-55 and 0.5, where ``b - a`` rounds to 0.5, so numpy's
    ``a + (b - a) t`` is 0.125 + 2^-55 and the other branch's ``b - (b - a)(1 - t)`` is 0.125; q25 is 0."""
    k = 81
    p_col, r_col = k - 2, k - 1
    X = np.zeros((8, k), dtype=np.float64)

    def put(row, plus, minus):
        X[row, list(plus)] = 1.0
        X[row, list(minus)] = -1.0

    put(0, (0, 1), (2, 3))
    put(6, (0, 1), (2, 3))        # corr(0, 6) = 1
    put(2, (4, 5), (6, 7))
    put(3, (4, 5), (6, 7))        # corr(2, 3) = 1
    put(4, (8, 9), (10, 11))
    put(5, (8, 9), (12, 13))      # corr(4, 5) = 0.5
    put(7, (14, 15), (12, 13))    # corr(5, 7) = 0.5, corr(4, 7) = 0
    put(1, list(range(16, 47)) + [p_col], range(47, 79))  # N = 64
    X[0, p_col] = 2.0 ** -51
    X[0, r_col] = -(2.0 ** -51)
    z = X / np.sqrt((X * X).sum(axis=1, keepdims=True))  # (cell 0's squared norm rounds to 4)
    C = z @ z.T
    assert C[0, 1] == 2.0 ** -55 and C[0, 0] == 1.0
    # offsets and scales on the cells that do not carry the tiny entries
    e = np.array([0, 2, -1, 0, 1, -2, 3, 0])
    c = np.array([0, 3, -5, 0, 7, 1, -2, 4])
    X = X * np.ldexp(1.0, e)[:, None] + c[:, None]
    X32 = X.astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), X)
    return X32, C


# --------------------------------------------------------------------------------------------------------------- #
# distances
# --------------------------------------------------------------------------------------------------------------- #
def dist_case(n, d, seed, dup=0, lim=7, off=50):
    """(X float32 n x d, Zc int64 n x d): X = Zc + per-column integer offsets, rows of Zc shuffled from
    ``vstack(A, -A)`` (+ a zero row when n is odd), A integer in [-lim, lim]; ``dup`` rows of A repeat earlier ones
    (so the matrix has exact zeros off the diagonal)."""
    rng = np.random.default_rng(seed)
    h = n // 2
    A = rng.integers(-lim, lim + 1, (h, d), dtype=np.int64)
    if dup and h > 1:
        src = rng.integers(0, h, min(dup, h - 1))
        A[h - len(src):] = A[src]
    Zc = np.vstack([A, -A] + ([np.zeros((1, d), dtype=np.int64)] if n % 2 else []))
    Zc = Zc[rng.permutation(n)]
    X = (Zc + rng.integers(-off, off + 1, (1, d))).astype(np.float32)
    assert float(np.abs(Zc).sum(axis=1).max(initial=0) * lim) < 2 ** 24 / 4
    return X, Zc


def exact_sqdist(Zc, rows=None):
    """Exact squared Euclidean distances of the rows ``rows`` (default all) to all rows: int64."""
    nrm = (Zc * Zc).sum(axis=1)
    R = Zc if rows is None else Zc[np.asarray(rows)]
    nr = nrm if rows is None else nrm[np.asarray(rows)]
    # the Gram through float64 BLAS: integer partial sums far below 2^53, so exact (int64 matmul has no BLAS)
    G = (R.astype(np.float64) @ Zc.T.astype(np.float64)).astype(np.int64)
    return nr[:, None] + nrm[None, :] - 2 * G


def dyadic_cnv(n, k, seed, density=0.3):
    """X_cnv-like float64 values: multiples of 1/8 with |x| <= 3, a fraction ``density`` nonzero (every sum of
    them is exact in float32 and float64)."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-24, 25, (n, k)) / 8.0
    return np.where(rng.random((n, k)) < density, v, 0.0)

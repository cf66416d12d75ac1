"""numpy oracle of the Ward linkage rounds: DESIGN.md section 5 restated (the specification of ``icv_ward_linkage``).

Input: an n x n float32 matrix of SQUARED distances, symmetric, zero diagonal, entries finite or +inf.  The linkage
matrix and the round count are a pure function of it:

round 0      every row searches its nearest alive column other than itself: the lexicographic minimum of
             (float32 value, slot); +inf is no neighbour (a row of +inf has none, nn = -1);
pairs        over the alive slots in ascending order: (r, c) is a pair iff c = nn[r] > r and nn[c] == r; it is
             logged as (r, c, dmin[r], size_r + size_c); slot r survives, c dies;
bystander    merged row r (r absorbed j), column c that did not merge:
                 v = ((double)(n_r+n_c) d_rc + (double)(n_j+n_c) d_jc - (double)n_c d_rj) / (double)(n_r+n_j+n_c)
             on the float32 operands widened to float64, left to right, no fused multiply-add;
             v > 0 ? (float)v : 0, written to D[r][c] and D[c][r];
same round   entry between two clusters merged in the same round: the merge of the lower surviving slot is applied
             first (to both parts of the other cluster, old sizes), then the other merge with the first cluster's
             new size;
neighbours   a merged row searches all alive columns; a row that did not merge keeps its cached (nn, dmin) unless
             the cached neighbour merged or died (or it has none): only then is it searched again;
no pair      every alive row is searched again; that pass is no round of its own (the round that found no pair
             is counted); a second round without a pair in a row: ValueError("... distances are not finite");
finish       height = sqrt((double)d2), raised to the heights already recorded for its two slots; stable sort by
             height; scipy ids from the slot -> cluster map, the smaller id first; sizes from the log.

Vectorised per round (the merged rows of a round are one P x n float64 block, the same-round entries P x P blocks);
it never calls the library.
"""
from __future__ import annotations

import numpy as np


def lw(dac, dbc, dab, na, nb, nc):
    """Lance-Williams update of a squared Ward distance: float32 operands, one float64 expression, float32 result."""
    f8 = np.float64
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(na + nb + nc).astype(f8)
        v = np.asarray(na + nc).astype(f8) * np.asarray(dac, dtype=np.float32).astype(f8)
        v = v + np.asarray(nb + nc).astype(f8) * np.asarray(dbc, dtype=np.float32).astype(f8)
        v = v - np.asarray(nc).astype(f8) * np.asarray(dab, dtype=np.float32).astype(f8)
        v = v / t
        return np.where(v > 0.0, v.astype(np.float32), np.float32(0.0)).astype(np.float32)


def _search(M, rows):
    """(nn, dmin) of the rows `rows` of the working matrix (diagonal and dead columns at +inf): the lexicographic
    minimum of (value, column); columns stay in ascending slot order, so the first of equal values is the lowest slot."""
    if 2 * len(rows) > M.shape[0]:  # most rows: no copy of the block
        nn = np.argmin(M, axis=1)[rows]
        dmin = M[rows, nn]
    else:
        blk = M[rows]
        nn = np.argmin(blk, axis=1)
        dmin = blk[np.arange(len(rows)), nn]
    return np.where(dmin < np.inf, nn, -1), dmin


def finish(n, li, lj, ld, ls, stats=None):
    """Merge log (slots kept / absorbed, float32 squared distances, sizes) -> scipy linkage matrix."""
    m = n - 1
    height = np.empty(m, dtype=np.float64)
    slot_h = np.zeros(n, dtype=np.float64)
    merged = np.zeros(n, dtype=bool)  # the slot holds a cluster of more than one leaf
    tied = 0
    for p in range(m):
        i, j = li[p], lj[p]
        h = max(float(np.sqrt(np.float64(ld[p]))), slot_h[i], slot_h[j])
        tied += int((merged[i] and slot_h[i] == h) or (merged[j] and slot_h[j] == h))
        height[p] = h
        slot_h[i] = h
        merged[i] = True
    order = np.argsort(height, kind="stable")
    cluster = np.arange(n, dtype=np.int64)
    Z = np.empty((m, 4), dtype=np.float64)
    for q, p in enumerate(order):
        a, b = cluster[li[p]], cluster[lj[p]]
        Z[q] = (min(a, b), max(a, b), height[p], ls[p])
        cluster[li[p]] = n + q
    if stats is not None:
        stats["parent_at_child_height"] = tied
    return Z


def ward_rounds(D32, stats=None):
    """(Z, rounds) of an n x n float32 squared-distance matrix.  ``stats`` (a dict) receives ``pairless_passes`` (how
    often every row had to be searched again) and ``parent_at_child_height`` (merges whose height equals that of a
    merge they contain)."""
    M = np.array(D32, dtype=np.float32, order="C")  # a copy: the rounds overwrite it
    n = M.shape[0]
    assert M.shape == (n, n) and n >= 1
    assert np.array_equal(M, M.T) and not M.diagonal().any(), "symmetric with a zero diagonal"
    if n == 1:
        return np.empty((0, 4)), 0
    # Storage only: the diagonal and the columns of dead slots are kept at +inf (never a neighbour), and the dead
    # rows and columns are dropped when they are the majority; `slot` names the slot of every kept row, ascending.
    np.fill_diagonal(M, np.inf)
    slot = np.arange(n)
    alive = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    nn, dmin = _search(M, np.arange(n))
    li, lj, ld, ls = [], [], [], []
    rounds = pairless = 0
    retry = False
    while alive.sum() > 1:
        if 2 * alive.sum() < len(slot):
            keep = np.flatnonzero(alive)
            new_pos = np.full(len(slot), -1)
            new_pos[keep] = np.arange(len(keep))
            M = np.ascontiguousarray(M[np.ix_(keep, keep)])
            slot, size, dmin = slot[keep], size[keep], dmin[keep]
            nn = np.where(nn[keep] >= 0, new_pos[np.maximum(nn[keep], 0)], -1)  # cached neighbours are alive
            alive = np.ones(len(keep), dtype=bool)
        rounds += 1
        live = np.flatnonzero(alive)
        c_of = nn[live]
        is_pair = (c_of > live) & (nn[np.maximum(c_of, 0)] == live)
        R, C = live[is_pair], c_of[is_pair]  # ascending in R: slot order
        if len(R) == 0:
            if retry:
                raise ValueError("ward_linkage: distances are not finite")
            retry = True
            pairless += 1
            nn[live], dmin[live] = _search(M, live)
            continue
        retry = False
        pd = dmin[R].copy()
        sr, sj = size[R], size[C]
        li += slot[R].tolist()
        lj += slot[C].tolist()
        ld += pd.tolist()
        ls += (sr + sj).tolist()
        # columns that did not merge
        by = alive.copy()
        by[R] = False
        by[C] = False
        U = np.flatnonzero(by)
        V = lw(M[np.ix_(R, U)], M[np.ix_(C, U)], pd[:, None], sr[:, None], sj[:, None], size[U][None, :])
        # clusters merged in the same round: [p, q] with p's merge first, used where R[p] < R[q]
        xk = lw(M[np.ix_(R, R)], M[np.ix_(C, R)], pd[:, None], sr[:, None], sj[:, None], sr[None, :])
        xl = lw(M[np.ix_(R, C)], M[np.ix_(C, C)], pd[:, None], sr[:, None], sj[:, None], sj[None, :])
        X = lw(xk, xl, pd[None, :], sr[None, :], sj[None, :], (sr + sj)[:, None])
        X = np.triu(X, 1)
        X = X + X.T
        X[np.arange(len(R)), np.arange(len(R))] = np.inf
        M[np.ix_(R, U)] = V
        M[np.ix_(U, R)] = V.T
        M[np.ix_(R, R)] = X
        M[:, C] = np.inf
        size[R] = sr + sj
        alive[C] = False
        # neighbours: the merged rows, and the rows whose cached neighbour merged or died
        touched = np.zeros(len(slot), dtype=bool)
        touched[R] = True
        touched[C] = True
        again = U[(nn[U] < 0) | touched[np.maximum(nn[U], 0)]]
        rows = np.concatenate([R, again])
        nn[rows], dmin[rows] = _search(M, rows)
    if stats is not None:
        stats["pairless_passes"] = pairless
    return finish(n, np.array(li), np.array(lj), np.array(ld, dtype=np.float32), np.array(ls), stats), rounds


def leaf_hashes(Z):
    """One 64-bit hash per merge of a linkage matrix: the sum (mod 2^64) of fixed random keys of its leaves."""
    n = Z.shape[0] + 1
    key = np.random.RandomState(0).randint(1, 2 ** 62, size=n, dtype=np.int64).astype(np.uint64)
    h = np.concatenate([key, np.zeros(n - 1, dtype=np.uint64)])
    with np.errstate(over="ignore"):
        for q in range(n - 1):
            h[n + q] = h[int(Z[q, 0])] + h[int(Z[q, 1])]
    return set(h[n:].tolist())


def leaf_sets(Z):
    """The leaf set of every merge of a linkage matrix, as frozensets, in row order."""
    n = Z.shape[0] + 1
    sets = [frozenset([i]) for i in range(n)]
    for q in range(n - 1):
        sets.append(sets[int(Z[q, 0])] | sets[int(Z[q, 1])])
    return sets[n:]

"""Numpy / pure-Python oracle of tl.cnv_changepoints, and the builders of its test cases.

The rules, implemented literally with Python floats (IEEE float64, no fused multiply-add) and explicit loops.  For one row
and one chromosome with the windows ``[s0, s1)``, ``L = s1 - s0``, the values ``x_1 .. x_L`` (an entry that is not stored
is 0.0), the penalty ``beta >= 0`` and the shortest segment ``m >= 1``:

1. Prefix chains.  ``P_0 = Q_0 = +0.0``, ``P_j = P_{j-1} + x_j``, ``Q_j = Q_{j-1} + x_j x_j``, ascending and sequential.
   The chain starts at +0.0 (``np.cumsum`` starts at ``x_1``: a row that begins with -0.0 gives -0.0 there), so a zero
   adds nothing and CSR, CSC, dense and stored zeros of either sign give the same bytes.
2. Cost of the segment ``(i, j]``: ``d = P_j - P_i``, ``c = (Q_j - Q_i) - (d d) / float(j - i)``; a ``c < 0.0`` becomes
   0.0.  The division is the correctly rounded one.
3. ``F_0 = 0.0``; ``F_j = min over the admissible i of ((F_i + c(i, j)) + beta)``.  ``i`` is admissible when
   ``(i == 0 or i >= m) and j - i >= m``; ``i = 0, j = L`` always is (a chromosome shorter than ``m`` is one segment).  A
   ``j`` without an admissible ``i`` has ``F_j = +inf`` and is never chosen as a predecessor.  The minimum is the smallest
   value, ties go to the lowest ``i``: a total order on ``(value, i)``.
4. Backtrack from ``L``; the segment ``(i, j]`` has the level ``(P_j - P_i) / float(j - i)``.
5. ``levels[s0 + i .. s0 + j)`` = the segment's level (n x W float64); ``starts[w] = 1`` at the first window of every
   segment, else 0 (n x W uint8).
6. Host scalars.  ``beta = (penalty (sigma sigma)) log(W)``.  ``sigma=None``: ``sqrt(D / (2 M))``, ``D = fsum(d_r)``,
   ``d_r`` = the sum over the chromosomes in ascending order, from +0.0, of each chromosome's chain, from +0.0, of
   ``(x_{t+1} - x_t)^2`` over its adjacent windows; ``M = n (W - C)``; ``M = 0`` gives sigma = 0, and sigma = 0 gives
   beta = 0.
7. Refusals.  A non-finite stored value is a ``ValueError``; with ``a`` the largest magnitude, so are an ``(a a) W``, an
   ``(a W) (a W)`` or a ``beta W`` that is not finite.  No ``d d`` overflows and no ``inf - inf`` arises in rule 2 then.
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

MAX_CHR_WINDOWS = 4096  # ICV_CHANGEPOINT_MAX_CHR_WINDOWS of include/infercnv_hip.h


# ---- rule 1 --------------------------------------------------------------------------------------------------------------
def prefix_chains(xs):
    """(P, Q) of rule 1: two lists of L + 1 Python floats."""
    P, Q = [0.0], [0.0]
    for x in xs:
        P.append(P[-1] + x)
        Q.append(Q[-1] + x * x)
    return P, Q


# ---- rules 2-3 -----------------------------------------------------------------------------------------------------------
def segment_cost(P, Q, i, j):
    d = P[j] - P[i]
    c = (Q[j] - Q[i]) - (d * d) / float(j - i)
    if c < 0.0:
        c = 0.0
    return c


def admissible(i, j, L, m):
    return (i == 0 and j == L) or ((i == 0 or i >= m) and j - i >= m)


def partition(xs, beta, m):
    """(F, back, P) of rule 3 in its scalar form: i ascends and only a strictly smaller value replaces."""
    L = len(xs)
    P, Q = prefix_chains(xs)
    F, back = [0.0] + [math.inf] * L, [0] * (L + 1)
    for j in range(1, L + 1):
        best, who = math.inf, 0
        for i in range(0, j):
            if not admissible(i, j, L, m):
                continue
            v = (F[i] + segment_cost(P, Q, i, j)) + beta
            if v < best:
                best, who = v, i
        F[j], back[j] = best, who
    return F, back, P


def partition_vectorised(xs, beta, m):
    """The same (F, back, P), the candidates of one j formed at once by numpy: the same operations on the same operands,
    and ``argmin`` takes the first of equal values, the lowest i."""
    L = len(xs)
    P, Q = prefix_chains(xs)
    Pa, Qa = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    F, back = np.full(L + 1, np.inf), [0] * (L + 1)
    F[0] = 0.0
    for j in range(1, L + 1):
        idx = np.arange(m, j - m + 1, dtype=np.int64)
        if j >= m or j == L:
            idx = np.concatenate([np.zeros(1, dtype=np.int64), idx])
        if idx.shape[0] == 0:
            continue
        d = Pa[j] - Pa[idx]
        with np.errstate(over="ignore", invalid="ignore"):
            c = (Qa[j] - Qa[idx]) - (d * d) / (j - idx).astype(np.float64)
            c = np.where(c < 0.0, 0.0, c)
            v = (F[idx] + c) + beta
        k = int(np.argmin(v))
        if v[k] < math.inf:
            F[j], back[j] = v[k], int(idx[k])
    return F.tolist(), back, P


# ---- rule 3 as the kernel shares it out ----------------------------------------------------------------------------------
LANES = 64  # lanes of the wavefront that takes one (row, chromosome) in k_changepoint_levels
NO_CANDIDATE = 0x7fffffff
LANE_MODES = ("kernel", "lane_le", "lowest_lane", "highest_i", "no_clamp")


def lane_partition(xs, beta, m, mode="kernel"):
    """(F, back, P) of rule 3 formed the way k_changepoint_levels forms it (csrc/icv_changepoint.hpp): the admissible i of
    one j are numbered k = 0 (i = 0, where ``with_zero`` admits it), 1, 2, ... (i = m + k - 1); lane l of 64 walks
    k = l, l + 64, ... and keeps its own best under a strict <; the least of the 64 bests is found, and among the lanes
    that hold it the lowest i.  ``mode`` "kernel" is that; every other mode is one mistake the kernel could make:

    - "lane_le": a lane replaces its best on <= (the highest of a lane's equal candidates survives);
    - "lowest_lane": among the lanes that hold the least value the lowest lane wins, not the lowest i;
    - "highest_i": ties go to the highest i, inside a lane and across the lanes;
    - "no_clamp": rule 2 without ``c < 0.0 -> 0.0``.

    It exists so that a host test can show which case tells the kernel from which mutant."""
    assert mode in LANE_MODES
    L = len(xs)
    P, Q = prefix_chains(xs)
    F, back = [0.0] + [math.inf] * L, [0] * (L + 1)
    replace_equal = mode in ("lane_le", "highest_i")
    for j in range(1, L + 1):
        with_zero = j >= m or j == L
        n_cand = 1 + max(j - 2 * m + 1, 0)
        best, bi = [math.inf] * LANES, [NO_CANDIDATE] * LANES
        for k in range(0 if with_zero else 1, n_cand):  # (ascending k: every lane meets its own k in ascending order)
            lane = k % LANES
            i = 0 if k == 0 else m + k - 1
            d = P[j] - P[i]
            c = (Q[j] - Q[i]) - (d * d) / float(j - i)
            if c < 0.0 and mode != "no_clamp":
                c = 0.0
            v = (F[i] + c) + beta
            if v < best[lane] or (replace_equal and v == best[lane]):
                best[lane], bi[lane] = v, i
        least = min(best)
        holders = [bi[lane] for lane in range(LANES) if best[lane] == least]  # (in ascending lane order)
        if mode == "lowest_lane":
            who = holders[0]
        elif mode == "highest_i":
            who = max([i for i in holders if i != NO_CANDIDATE], default=NO_CANDIDATE)
        else:
            who = min(holders)
        F[j], back[j] = least, 0 if who == NO_CANDIDATE else who
    return F, back, P


# ---- rules 4-5 -----------------------------------------------------------------------------------------------------------
def backtrack(back, L):
    """The segments (i, j] of rule 4, ascending."""
    out, j = [], L
    while j > 0:
        i = back[j]
        assert 0 <= i < j
        out.append((i, j))
        j = i
    out.reverse()
    return out


def segment_chromosome(xs, beta, m, vectorised=False, part=None):
    """(levels, starts, segments, cost) of one chromosome: two lists of L entries, the list of (i, j] and F_L.  ``part``: a
    function like ``partition`` to take rule 3 from instead (the lane model below and its mutants)."""
    xs = [float(v) for v in xs]
    L = len(xs)
    F, back, P = (part or (partition_vectorised if vectorised else partition))(xs, float(beta), int(m))
    segs = backtrack(back, L)
    levels, starts = [0.0] * L, [0] * L
    for i, j in segs:
        level = (P[j] - P[i]) / float(j - i)
        for t in range(i, j):
            levels[t] = level
        starts[i] = 1
    return levels, starts, segs, F[L]


# ---- rule 6 --------------------------------------------------------------------------------------------------------------
def rows_of(x):
    """The rows of a scipy sparse matrix or a dense array as lists of W Python floats, stored values as they are (a stored
    -0.0 stays -0.0), every other entry +0.0."""
    if sp.issparse(x):
        x = x.tocsr()
        n, w = x.shape
        data, indices, indptr = x.data.astype(np.float64).tolist(), x.indices.tolist(), x.indptr.tolist()
        out = []
        for r in range(n):
            row = [0.0] * w
            for k in range(indptr[r], indptr[r + 1]):
                row[indices[k]] = data[k]
            out.append(row)
        return out
    return np.asarray(x, dtype=np.float64).tolist()


def bounds(chr_pos, n_windows):
    return sorted(int(v) for v in chr_pos.values()) + [int(n_windows)]


def diffsq(rows, edges):
    """d_r of rule 6: list of n Python floats."""
    out = []
    for row in rows:
        d = 0.0
        for s0, s1 in zip(edges[:-1], edges[1:]):
            e = 0.0
            for t in range(s0, s1 - 1):
                dx = row[t + 1] - row[t]
                e = e + dx * dx
            d = d + e
        out.append(d)
    return out


def default_sigma(x, chr_pos):
    n, w = x.shape
    edges = bounds(chr_pos, w)
    pairs = n * (w - (len(edges) - 1))
    if pairs == 0:
        return 0.0
    return math.sqrt(math.fsum(diffsq(rows_of(x), edges)) / (2.0 * float(pairs)))


def penalty_of(penalty, sigma, n_windows):
    return (float(penalty) * (sigma * sigma)) * math.log(n_windows)


# ---- rule 7 --------------------------------------------------------------------------------------------------------------
def check_values(rows, beta, who="cnv_changepoints"):
    w = float(len(rows[0]))
    a = 0.0
    for row in rows:
        for v in row:
            if not math.isfinite(v):
                raise ValueError(f"{who}: non-finite values")
            a = max(a, abs(v))
    t = a * w
    if not (math.isfinite((a * a) * w) and math.isfinite(t * t)):
        raise ValueError(f"{who}: the value of magnitude {a!r} overflows float64")
    if not math.isfinite(beta * w):
        raise ValueError(f"{who}: beta overflows float64")


# ---- the whole function ----------------------------------------------------------------------------------------------------
def cnv_changepoints(x, chr_pos, penalty=2.0, sigma=None, min_windows=1, vectorised=True, part=None):
    """dict(levels float64 n x W, starts uint8 n x W, n_segments int32 n, sigma, beta, table) of rules 1-7; ``table`` is the
    list of (cell, chromosome, start, end, n_windows, mean) ordered by (cell, start).  ``part``: as for
    ``segment_chromosome``."""
    n, w = x.shape
    rows = rows_of(x)
    edges = bounds(chr_pos, w)
    names = [k for k, _ in sorted(chr_pos.items(), key=lambda kv: int(kv[1]))]
    if sigma is None:
        sigma = default_sigma(x, chr_pos)
    sigma = float(sigma)
    beta = penalty_of(penalty, sigma, w)
    check_values(rows, beta)
    levels = np.zeros((n, w), dtype=np.float64)
    starts = np.zeros((n, w), dtype=np.uint8)
    table = []
    for r, row in enumerate(rows):
        for c, (s0, s1) in enumerate(zip(edges[:-1], edges[1:])):
            lv, st, segs, _ = segment_chromosome(row[s0:s1], beta, min_windows, vectorised, part)
            levels[r, s0:s1] = lv
            starts[r, s0:s1] = st
            table.extend((r, names[c], s0 + i, s0 + j, j - i, lv[i]) for i, j in segs)
    return {"levels": levels, "starts": starts, "n_segments": starts.sum(axis=1, dtype=np.int64).astype(np.int32),
            "sigma": sigma, "beta": beta, "table": table}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- case builders ---------------------------------------------------------------------------------------------------------
def chr_pos_of(lengths):
    """{"chr1": 0, "chr2": len_1, ...}, inserted in shuffled order (the function sorts by start, not by name)."""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    order = list(range(len(lengths)))
    order = order[1::2] + order[0::2]
    return {f"chr{c + 1}": int(starts[c]) for c in order}


PLANTED_STARTS = (0, 90, 150, 200)
PLANTED_WINDOWS = 270
PLANTED_EVENTS = ((20, 50, 0.3), (100, 130, 0.6), (160, 175, -0.3), (230, 236, 0.6))
PLANTED_SEGMENTS = 72  # 6 rows x (3 + 3 + 3 + 3): every event lies inside its chromosome


def planted_truth():
    """(truth levels of one row, the sorted true segment starts of one row)."""
    level = np.zeros(PLANTED_WINDOWS)
    cuts = set(PLANTED_STARTS)
    for a, b, v in PLANTED_EVENTS:
        level[a:b] = v
        cuts.update((a, b))
    return level, sorted(cuts)


def planted(seed):
    """The planted case: 6 rows, 270 windows, chromosomes starting at 0, 90, 150, 200; levels 0.3 on [20, 50), 0.6 on
    [100, 130), -0.3 on [160, 175), 0.6 on [230, 236), 0 elsewhere; noise N(0, 0.1).  dict(x dense, chr_pos, truth)."""
    level, _ = planted_truth()
    x = np.tile(level, (6, 1)) + np.random.default_rng(seed).normal(0, 0.1, (6, PLANTED_WINDOWS))
    return {"x": x, "chr_pos": {f"chr{k + 1}": s for k, s in enumerate(PLANTED_STARTS)}, "truth": np.tile(level, (6, 1))}


def planted_figures(x_truth, levels, starts):
    """What the planted case asserts, from the found levels and starts: dict(n_segments, shift, mean_error, off)."""
    level, cuts = planted_truth()
    n_segments, shift, mean_error = int(starts.sum()), 0, 0.0
    for r in range(starts.shape[0]):
        found = np.flatnonzero(starts[r]).tolist()
        if len(found) == len(cuts):
            shift = max(shift, max(abs(a - b) for a, b in zip(found, cuts)))
        else:
            shift = PLANTED_WINDOWS
        for a, b in zip(cuts, cuts[1:] + [PLANTED_WINDOWS]):  # the found level at the middle of every planted segment
            mean_error = max(mean_error, abs(float(levels[r, (a + b) // 2]) - float(level[a])))
    off = int((np.abs(levels - x_truth) > 0.15).sum())
    return {"n_segments": n_segments, "shift": shift, "mean_error": mean_error, "off": off}


MIXED_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


def steps(n, lengths, seed, noise=0.1, density=1.0):
    """n rows over the chromosomes of ``lengths``: noise N(0, noise) on piecewise-constant levels with a change every
    5 .. 40 windows from {-0.6, -0.3, 0, 0.3, 0.6}; with ``density`` < 1 the rest is dropped (not stored).  Canonical CSR."""
    rng = np.random.default_rng(seed)
    w = int(sum(lengths))
    dense = rng.normal(0.0, noise, (n, w))
    for r in range(n):
        t = 0
        while t < w:
            run = int(rng.integers(5, 41))
            dense[r, t:t + run] += rng.choice([-0.6, -0.3, 0.0, 0.0, 0.3, 0.6])
            t += run
    if density < 1.0:
        dense[rng.random((n, w)) >= density] = 0.0
    return sp.csr_matrix(dense)


def exact_ties(lengths=(12, 7, 1, 9, 16)):
    """Rows whose values are multiples of 1/4 (every sum, square and mean below is exact), built so that several
    segmentations cost exactly the same: constant rows, alternating rows, symmetric steps, and an all-zero row."""
    w = int(sum(lengths))
    q = 0.25
    rows = [np.full(w, v) for v in (0.0, q, -q, 1.0)]
    rows += [np.where(np.arange(w) % 2 == 0, q, -q), np.where(np.arange(w) % 2 == 0, 0.0, 2 * q)]
    rows += [np.where(np.arange(w) % 4 < 2, 1.0, 0.0), np.where(np.arange(w) % 6 < 3, -q, q)]
    rng = np.random.default_rng(3)
    rows += [rng.integers(-2, 3, size=w) * q for _ in range(6)]
    return sp.csr_matrix(np.stack(rows)), chr_pos_of(lengths)


def shuffled_rows(x, seed):
    """(indptr int64, indices int32, data float64) of the canonical CSR matrix ``x`` with the entries of every row in an
    order of their own (a permutation seeded per row): the same matrix, its columns unique and not sorted."""
    x = x.tocsr()
    indices, data = x.indices.astype(np.int32), x.data.astype(np.float64)
    for r in range(x.shape[0]):
        a, b = int(x.indptr[r]), int(x.indptr[r + 1])
        order = np.random.default_rng([seed, r]).permutation(b - a)
        indices[a:b], data[a:b] = indices[a:b][order], data[a:b][order]
    return x.indptr.astype(np.int64), indices, data


@functools.lru_cache(maxsize=None)
def expected(name):
    """The named GPU case with the oracle's answer, computed once: dict(x, chr_pos, kwargs, want)."""
    c = CASES[name]()
    c["want"] = cnv_changepoints(c["x"], c["chr_pos"], **c["kwargs"])
    for v in (c["want"]["levels"], c["want"]["starts"], c["want"]["n_segments"]):
        v.setflags(write=False)
    return c


def _case(x, lengths, **kwargs):
    return {"x": x, "chr_pos": chr_pos_of(lengths), "kwargs": kwargs}


def _empty_row():
    x = steps(4, (40, 9, 70), 21, density=0.4).toarray()
    x[1] = 0.0
    return _case(sp.csr_matrix(x), (40, 9, 70))


def _ties(lengths=None, **kwargs):
    x, chr_pos = exact_ties() if lengths is None else exact_ties(lengths)
    return {"x": x, "chr_pos": chr_pos, "kwargs": kwargs}


# Chromosomes in which a lane of the kernel has a second (65, 129) and up to a fourth (200) candidate and the candidates
# lie in all four rows of 16 lanes; 64 is the longest in which every lane still has at most one.
TIES_LONG_LENGTHS = (65, 129, 200, 64)
# The penalty that makes beta exactly 1/8 at sigma = 0.5 and W = 458: (penalty 0.25) log(458) rounds to 0.125.  A beta of
# the form c log(W) with a dyadic c, as in "ties", "ties_m3" and "ties_long_m3", is no multiple of 1/4: F_j = cost + k beta
# is rounded differently along different segmentations, and the best one of every such row is the only best one in float64
# (tests/test_changepoint_oracle.py records it): those cases cannot tell one tie rule from another, this one can.
EIGHTH_PENALTY = 0.08160774858657104

CLAMP_VALUES = (0.1, 0.3, -0.7, 1.0 / 3.0, 1e-3, 123.456)
CLAMP_LENGTHS = (65, 130)
TINY_BETA = {"sigma": 1e-10, "penalty": 1.0}  # beta = 1e-20 log(195) = 5.3e-20: far below every cost that is more than rounding


def _clamp_constant_rows(**kwargs):
    """Values that are no multiples of a power of two, as constant rows and as two plateaus (v, then 3 v, the step in the
    middle of every chromosome): the cost of a constant stretch is 0 but for the rounding of Q and of (d d) / n, which
    leaves some of them below 0.0 -- the clamp of rule 2 decides what the ties between the segmentations look like."""
    w = int(sum(CLAMP_LENGTHS))
    step = np.concatenate([np.where(np.arange(n) < n // 2, 1.0, 3.0) for n in CLAMP_LENGTHS])
    rows = [np.full(w, v) for v in CLAMP_VALUES] + [v * step for v in CLAMP_VALUES]
    return _case(sp.csr_matrix(np.stack(rows)), CLAMP_LENGTHS, **kwargs)


EVERY_LANE_WINDOWS = 131


def _minimum_in_every_lane():
    """Row r - 1 (r = 1 .. 130) is 0.0 on [0, r) and 1.0 on [r, 131): with beta = log(131) / 16 the two exact pieces cost
    2 beta and everything else more, so the back-pointer of j = L is r and nothing else comes near it: candidate k = r,
    lane r % 64, in the first (r < 64), second and third (r >= 128) round of k."""
    w = EVERY_LANE_WINDOWS
    x = (np.arange(w)[None, :] >= np.arange(1, w)[:, None]).astype(np.float64)
    return _case(sp.csr_matrix(x), (w,), sigma=0.25, penalty=1.0, min_windows=1)


REFUSAL_BOUND_WINDOWS = 70
REFUSAL_BOUND_A = 3e151   # (a a) W = 6.3e304 and (a W) (a W) = 4.41e306: inside rule 7; 3e152 is outside


def _values_at_the_refusal_bound():
    w = REFUSAL_BOUND_WINDOWS
    rng = np.random.default_rng(23)
    a = REFUSAL_BOUND_A
    rows = [rng.choice([-a, a, 0.0, a / 2], size=w) for _ in range(3)]
    rows.append(rng.choice([-1e-160, 1e-160, 0.0, 0.5e-160], size=w))  # the squares are subnormal
    rows.append(rng.choice([-5e-324, 5e-324], size=w))                  # the squares are 0.0: every cost is, all ties
    return _case(sp.csr_matrix(np.stack(rows)), (w,), penalty=0.0, sigma=1.0)


SEVENTY = tuple(int(v) for v in np.random.default_rng(5).integers(1, 12, size=70))
CASES = {
    "mixed_n3": lambda: _case(steps(3, MIXED_LENGTHS, 11), MIXED_LENGTHS),
    "mixed_n1": lambda: _case(steps(1, MIXED_LENGTHS, 12, density=0.5), MIXED_LENGTHS),
    "mixed_n70": lambda: _case(steps(70, (1, 2, 63, 64, 65), 13, density=0.3), (1, 2, 63, 64, 65)),
    "chromosomes_70": lambda: _case(steps(3, SEVENTY, 14), SEVENTY),
    "m2": lambda: _case(steps(3, MIXED_LENGTHS, 15), MIXED_LENGTHS, min_windows=2),
    "m5": lambda: _case(steps(3, MIXED_LENGTHS, 16), MIXED_LENGTHS, min_windows=5),
    "m_is_L": lambda: _case(steps(3, (64, 30, 64), 17), (64, 30, 64), min_windows=64),
    "m_is_L_plus_1": lambda: _case(steps(3, (64, 30, 64), 17), (64, 30, 64), min_windows=65),
    "m_half_L": lambda: _case(steps(3, (64, 30, 65), 18), (64, 30, 65), min_windows=32),
    "beta_0": lambda: _case(steps(3, (1, 2, 63, 130), 19), (1, 2, 63, 130), penalty=0.0),
    "beta_huge": lambda: _case(steps(3, (1, 2, 63, 130), 20), (1, 2, 63, 130), penalty=1e12),
    "empty_row": _empty_row,
    "ties": lambda: _ties(sigma=0.25, penalty=1.0),
    "ties_beta_0": lambda: _ties(penalty=0.0),
    "ties_m3": lambda: _ties(sigma=0.5, penalty=0.5, min_windows=3),
    "chromosome_4096": lambda: _case(steps(1, (MAX_CHR_WINDOWS, 5), 22, density=0.5), (MAX_CHR_WINDOWS, 5)),
    # the limits of the lane share-out, of the clamp and of rule 7 (tests/test_changepoint_oracle.py shows on the host what
    # each of them tells apart)
    "ties_long": lambda: _ties(TIES_LONG_LENGTHS, penalty=0.0),
    "ties_long_m2": lambda: _ties(TIES_LONG_LENGTHS, penalty=0.0, min_windows=2),
    "ties_long_m3": lambda: _ties(TIES_LONG_LENGTHS, sigma=0.5, penalty=0.5, min_windows=3),
    "ties_long_m3_beta_eighth": lambda: _ties(TIES_LONG_LENGTHS, sigma=0.5, penalty=EIGHTH_PENALTY, min_windows=3),
    "clamp_constant_rows": lambda: _clamp_constant_rows(penalty=0.0),
    "clamp_constant_rows_tiny_beta": lambda: _clamp_constant_rows(**TINY_BETA),
    "minimum_in_every_lane": _minimum_in_every_lane,
    "values_at_the_refusal_bound": _values_at_the_refusal_bound,
}
EDGE_CASES = ("ties_long", "ties_long_m2", "ties_long_m3", "ties_long_m3_beta_eighth", "clamp_constant_rows",
                   "clamp_constant_rows_tiny_beta", "minimum_in_every_lane", "values_at_the_refusal_bound")
TIES_CASES = ("ties", "ties_beta_0", "ties_m3", "ties_long", "ties_long_m2", "ties_long_m3", "ties_long_m3_beta_eighth")
TIES_CASES_WITHOUT_A_TIE = ("ties", "ties_m3", "ties_long_m3")  # beta = c log(W): see EIGHTH_PENALTY

"""The written contract of tl.cnv_rank_groups, restated: rule 2 with Python ints from the two counts,
rules 3-4 with one correctly rounded float64 operation after the other.

  1. an entry that is not stored is 0; a stored 0.0 or -0.0 is the same 0; a float32 is used as the float64 it converts
     to; a non-finite value is refused (flag bit 0).
  2. per window, over the N cells of the population (code >= 0): 2 r_i = #{x_j < x_i} + #{x_j <= x_i} + 1;
     R2[g,w] = the sum of 2 r_i over the cells of group g; T[w] = the sum over the distinct values of c^3 - c.
  3. n1 = n_g, n2 = N - n1: U2 = R2 - n1 (n1 + 1), D2 = U2 - n1 n2 (exact); k = float(N^3 - N - T);
     var = (float(n1 n2) k) / float(12 N (N - 1)); z = (float(D2) / 2) / sqrt(var); p = erfc(|z| / sqrt(2));
     auc = float(U2) / float(2 n1 n2); k == 0 or n2 == 0 gives z = 0, p = 1, and auc = 0.5 when n2 == 0.
  4. Benjamini-Hochberg over the W windows of a group: stable ascending sort, p W / rank, running minimum from the right,
     clipped at 1.

The kernel's sizes are restated here (WAVE, SUM_THREADS, CHUNK) because the limit cases are built around them.
"""
import math

import numpy as np
import scipy.sparse as sp
from scipy.special import erfc

WAVE = 64            # lanes of a wavefront
SUM_THREADS = 256    # threads per workgroup of the rank sums (csrc/icv_rank.hpp: kRkSumThreads)
CHUNK = 2048         # sorted entries per workgroup of the rank sums (kRkChunk)
SLAB = 128           # rows per workgroup of the count and the scatter (kRkSlab)
TILE = 8192          # windows per workgroup of the count and the scatter (kRkTile)
LDS_GROUPS = 2048    # codes whose sums a workgroup of the rank sums keeps in LDS (kRkLdsGroups); more go to global atomics
MAX_CELLS = 1 << 21


def dense_rows(x):
    """The matrix as a dense float64 array by rule 1 (duplicates of a sparse matrix are summed by scipy, as the package's
    intake does)."""
    if sp.issparse(x):
        return np.asarray(x.astype(np.float64).toarray())
    return np.asarray(x).astype(np.float64)


def tables(x, code, n_groups):
    """(R2, T, flags): int64 ``n_groups x W`` and ``W`` of rule 2 for ``code`` (per row: -1 outside the population,
    0 .. n_groups - 1 a tested group, anything larger: ranked, in no tested group); flags bit 0 for a non-finite value
    of the population (the tables are None then)."""
    code = np.asarray(code, dtype=np.int64)
    cells = np.flatnonzero(code >= 0)
    pop = dense_rows(x)[cells]
    group = code[cells]
    w = pop.shape[1]
    if not np.isfinite(pop).all():
        return None, None, 1
    r2 = [[0] * w for _ in range(n_groups)]
    tie = [0] * w
    for j in range(w):
        col = pop[:, j] + 0.0  # (-0.0 + 0.0 = +0.0: one zero)
        ordered = np.sort(col)
        less = np.searchsorted(ordered, col, side="left")         # #{x_j < x}
        less_equal = np.searchsorted(ordered, col, side="right")  # #{x_j <= x}
        for i in range(col.shape[0]):
            if group[i] < n_groups:
                r2[int(group[i])][j] += int(less[i]) + int(less_equal[i]) + 1
        _, counts = np.unique(col, return_counts=True)
        tie[j] = sum(int(c) ** 3 - int(c) for c in counts)
    assert all(abs(v) < 2 ** 63 for row in r2 for v in row) and all(v < 2 ** 63 for v in tie)
    return np.asarray(r2, dtype=np.int64).reshape(n_groups, w), np.asarray(tie, dtype=np.int64), 0


def statistics(r2, tie, n_cells, n_pop):
    """(z, p, auc) of rule 3, element by element with Python ints and floats."""
    g_count, w = np.asarray(r2).shape
    z, p, auc = (np.zeros((g_count, w), dtype=np.float64) for _ in range(3))
    big_n = int(n_pop)
    for g in range(g_count):
        n1 = int(n_cells[g])
        n2 = big_n - n1
        for j in range(w):
            u2 = int(r2[g][j]) - n1 * (n1 + 1)
            d2 = u2 - n1 * n2
            k = float(big_n ** 3 - big_n - int(tie[j]))
            if n2 == 0:
                z[g, j], p[g, j], auc[g, j] = 0.0, 1.0, 0.5
                continue
            auc[g, j] = float(u2) / float(2 * n1 * n2)
            if k == 0.0:
                z[g, j], p[g, j] = 0.0, 1.0
                continue
            var = (float(n1 * n2) * k) / float(12 * big_n * (big_n - 1))
            z[g, j] = (float(d2) / 2.0) / math.sqrt(var)
            p[g, j] = float(erfc(abs(z[g, j]) / math.sqrt(2.0)))
    return z, p, auc


def adjust(p):
    """Rule 4, row by row."""
    p = np.asarray(p, dtype=np.float64)
    out = np.zeros_like(p)
    w = p.shape[1]
    for g in range(p.shape[0]):
        order = sorted(range(w), key=lambda j: p[g, j])  # (sorted is stable)
        low = math.inf
        for position in range(w - 1, -1, -1):
            q = float(p[g, order[position]]) * float(w) / float(position + 1)
            low = min(low, q)
            out[g, order[position]] = min(low, 1.0)
    return out


def regions(z, p_adj, auc, chr_starts, alpha, min_windows):
    """Rows (group index, start, end, direction, score, pvals_adj_max, auc) of the ``regions`` table: maximal runs, inside
    one chromosome, of windows with p_adj < alpha and one sign of z, ordered by (group, start)."""
    g_count, w = z.shape
    first = set(int(s) for s in chr_starts)
    sign = np.where(p_adj < alpha, np.sign(z), 0.0).astype(np.int64)
    rows = []
    for g in range(g_count):
        a = 0
        while a < w:
            if sign[g, a] == 0:
                a += 1
                continue
            b = a + 1
            while b < w and b not in first and sign[g, b] == sign[g, a]:
                b += 1
            if b - a >= min_windows:
                best = a
                for j in range(a, b):
                    if abs(z[g, j]) > abs(z[g, best]):
                        best = j
                rows.append((g, a, b, int(sign[g, a]), float(z[g, best]), float(max(p_adj[g, a:b])),
                             float(np.mean(auc[g, a:b]))))
            a = b
    return rows


def population(codes, n_groups, min_cells):
    """(code per row, kept group numbers, n_cells of the kept, N): the tested groups are renumbered 0 .. G - 1, the cells
    of the smaller ones get G, a missing label stays -1."""
    codes = np.asarray(codes, dtype=np.int64)
    sizes = np.bincount(codes[codes >= 0], minlength=n_groups)
    kept = np.flatnonzero(sizes >= min_cells)
    new = np.full(n_groups, len(kept), dtype=np.int64)
    new[kept] = np.arange(len(kept))
    code = np.where(codes >= 0, new[np.maximum(codes, 0)], -1)
    return code, kept, sizes[kept].astype(np.int64), int(sizes.sum())


def rank_groups(x, codes, n_groups, chr_starts, min_cells=2, alpha=0.05, min_windows=1):
    """dict of everything tl.cnv_rank_groups derives from the ranks, for the group numbers ``codes`` (-1: no label)."""
    code, kept, n_cells, n_pop = population(codes, n_groups, min_cells)
    r2, tie, flags = tables(x, code, len(kept))
    assert flags == 0
    z, p, auc = statistics(r2, tie, n_cells, n_pop)
    p_adj = adjust(p)
    return {"kept": kept, "n_cells": n_cells, "N": n_pop, "code": code, "R2": r2, "T": tie, "scores": z, "pvals": p,
            "pvals_adj": p_adj, "auc": auc, "regions": regions(z, p_adj, auc, chr_starts, alpha, min_windows)}


# ---- inputs shared by the CPU test of this oracle and the GPU tests -----------------------------------------------------------
def random_case(n=67, w=37, seed=1):
    """(x canonical float64 CSR with stored 0.0 and -0.0 and repeated values, codes): 4 groups and missing labels, group 4
    of one cell (below min_cells = 2).  The values are float32 numbers, so that every kind of input holds the same."""
    rng = np.random.default_rng(seed)
    dense = np.round(rng.normal(0.0, 0.5, (n, w)), 1) * (rng.random((n, w)) < 0.4)  # (one decimal: many ties)
    dense[:, 5] = rng.normal(0.0, 0.5, n)  # a window stored in every cell, no ties
    dense[:, 6] = 0.0                      # a window with nothing stored
    x = sp.csr_matrix(dense.astype(np.float32).astype(np.float64))
    pick = rng.choice(x.nnz, size=x.nnz // 15, replace=False)
    x.data[pick[::2]] = 0.0
    x.data[pick[1::2]] = -0.0
    codes = rng.integers(-1, 4, size=n)
    codes[11] = 4
    return x, codes


PLANTED_SIZES = (48, 48, 48, 96)                         # three clones and the normal cells
PLANTED_CHR = {"chr1": 0, "chr2": 90, "chr3": 150, "chr4": 210}
PLANTED_EVENTS = ((0, 20, 50, 1), (1, 100, 130, -1), (2, 200, 215, 1))  # (clone, first window, behind the last, sign)


def planted_clones(seed):
    """(x dense float64 240 x 270, codes, truth int8 4 x 270): noise 0.3, events of +-0.3, |x| < 0.15 set to 0."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((4, 270), dtype=np.int8)
    for g, a, b, s in PLANTED_EVENTS:
        truth[g, a:b] = s
    codes = np.repeat(np.arange(4), PLANTED_SIZES)[rng.permutation(sum(PLANTED_SIZES))]
    x = rng.normal(0.0, 0.3, (sum(PLANTED_SIZES), 270)) + 0.3 * truth[codes]
    x[np.abs(x) < 0.15] = 0.0
    return x, codes, truth


def planted_verdict(result, truth):
    """(missed, false_calls): the planted (group, window) pairs that are not significant with the planted sign, and the
    significant calls among the (group, window) pairs of the windows where no clone has an event."""
    call = np.where(result["pvals_adj"] < 0.05, np.sign(result["scores"]), 0.0).astype(np.int8)
    planted = truth != 0
    quiet = ~planted.any(axis=0)
    return int((call[planted] != truth[planted]).sum()), int((call[:, quiet] != 0).sum())


def run_column(n, run, start, seed, lower=True):
    """A column of n distinct-looking values of which ``run`` equal ones lie at the sorted positions [start, start + run):
    ``start`` smaller distinct values below them, the rest above; shuffled.  All positive unless ``lower`` puts the
    values below the run on the negative side."""
    rng = np.random.default_rng(seed)
    below = -(np.arange(start, 0, -1, dtype=np.float64)) if lower else 0.5 + np.arange(start) / (2.0 * max(start, 1))
    above = 3.0 + np.arange(n - start - run, dtype=np.float64)
    col = np.concatenate([below, np.full(run, 2.0), above])
    return col[rng.permutation(n)]


LDS_TABLE_CELLS = 2300  # above CHUNK: the segment of a window stored in every cell spans two workgroups of the rank sums


def lds_table_matrix():
    """2300 cells x 5 windows, dense float64: a window stored in every cell without ties, a run of 1025 equal values across
    the chunk boundary, one-decimal values of both signs at 40 % density, a window with nothing stored and a window of
    negatives only."""
    n = LDS_TABLE_CELLS
    rng = np.random.default_rng(31)
    x = np.zeros((n, 5))
    x[:, 0] = rng.normal(0.0, 1.0, n)
    assert np.unique(x[:, 0]).shape[0] == n and (x[:, 0] != 0).all()
    x[:, 1] = run_column(n, 1025, CHUNK - 500, seed=4)
    x[:, 2] = np.round(rng.normal(0.0, 0.5, n), 1) * (rng.random(n) < 0.4)
    x[:, 4] = -np.abs(rng.normal(0.0, 1.0, n)) - 0.1
    return x


def group_codes(n, n_groups, n_untested, n_outside, seed):
    """n codes in shuffled order: every tested group 0 .. G - 1 has a cell, the cells left over go to the first G // 500
    groups (sizes from 1 to a few dozen), ``n_untested`` cells have the code G (ranked, in no tested group) and
    ``n_outside`` the code -1."""
    rng = np.random.default_rng(seed)
    spare = n - n_groups - n_untested - n_outside
    assert spare >= 0
    code = np.concatenate([np.arange(n_groups), rng.integers(0, max(n_groups // 500, 1), size=spare),
                           np.full(n_untested, n_groups), np.full(n_outside, -1)])
    return code[rng.permutation(n)].astype(np.int64)


def lds_table_cases():
    """The number of codes, G tested groups and the code G of the rest, at and past what the rank sums keep in LDS: the
    last LDS slot in use (G + 1 == LDS_GROUPS), one code more (the form with global atomics per entry), and far more with
    cells outside the population."""
    x = lds_table_matrix()
    n = x.shape[0]
    return [("groups_fill_the_lds_table", x, group_codes(n, LDS_GROUPS - 1, 100, 0, seed=41), LDS_GROUPS - 1),
            ("groups_one_past_the_lds_table", x, group_codes(n, LDS_GROUPS, 100, 0, seed=42), LDS_GROUPS),
            ("groups_far_past_the_lds_table", x, group_codes(n, 2200, 90, 5, seed=43), 2200)]


def limit_cases():
    """[(name, x, code, n_groups)]: the limits of DESIGN.md 4.20; ``code`` as the engine binding takes it.  Every case is a
    handful of columns of 1 to about 2 300 cells."""
    cases = []
    rng = np.random.default_rng(7)
    # runs of equal values across the wavefront (64), workgroup-stride (256) and chunk (2048) positions of the sorted
    # segment: a run of R equal values that begins `before` positions in front of the boundary
    cols, n = [], 1100
    for run, start in ((63, 1), (64, 0), (64, 32), (65, 63), (255, 1), (256, 0), (256, 128), (257, 255), (1025, 40),
                       (63, WAVE - 31), (65, SUM_THREADS - 1), (257, 2 * SUM_THREADS - 100)):
        cols.append(run_column(n, run, start, seed=run * 1000 + start, lower=bool((run + start) % 2)))
    code = rng.integers(0, 3, size=n)
    cases.append(("runs_at_wave_and_workgroup_boundaries", np.stack(cols, axis=1), code, 3))
    # a run across the chunk boundary of the rank sums needs a segment above CHUNK entries
    n = CHUNK + 300
    cols = [run_column(n, 1025, CHUNK - 500, seed=1), run_column(n, 65, CHUNK - 1, seed=2, lower=False),
            run_column(n, 257, CHUNK - 256, seed=3)]
    cases.append(("runs_at_the_chunk_boundary", np.stack(cols, axis=1), rng.integers(0, 2, size=n), 2))
    # zeros of both signs, all-equal and one-sided columns, adjacent doubles, a subnormal, +-1e300
    n = 130
    x = np.zeros((n, 9))
    x[:, 1] = rng.normal(0, 1, n)                       # stored in every cell (column 0: nothing stored)
    x[:, 2] = 0.75                                      # one value in all cells
    x[:, 3] = -np.abs(rng.normal(0, 1, n)) - 0.1        # only negatives
    x[:, 4] = np.abs(rng.normal(0, 1, n)) + 0.1         # only positives
    x[: n // 2, 5] = rng.choice([1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0)], n // 2)  # adjacent doubles
    x[::3, 6] = rng.choice([5e-324, -5e-324, 2.2250738585072014e-308], len(x[::3, 6]))            # subnormals
    x[::4, 7] = rng.choice([1e300, -1e300, 1.0, -1.0], len(x[::4, 7]))
    x[::2, 8] = rng.choice([-1.5, 1.5], len(x[::2, 8]))  # a few negatives, zeros, a few positives
    cases.append(("values_dense", x, rng.integers(-1, 4, size=n), 4))
    s = sp.csr_matrix(x)
    s.data[rng.choice(s.nnz, size=s.nnz // 6, replace=False)] = -0.0   # a stored -0.0 is the zero, not a negative
    s.data[rng.choice(s.nnz, size=s.nnz // 6, replace=False)] = 0.0
    cases.append(("values_csr_signed_zeros", s, rng.integers(-1, 4, size=n), 4))
    only = sp.csr_matrix((np.asarray([-0.0, 0.0, -0.0, 2.0]), np.asarray([0, 0, 0, 0]), np.asarray([0, 1, 2, 3, 4])), shape=(4, 1))
    cases.append(("minus_zero_is_no_negative", only, np.asarray([0, 1, 0, 1]), 2))
    # groups of one cell, n2 == 0, descending group order, float32, W = 1 and N = 1
    x = np.round(rng.normal(0, 1, (9, 3)), 0)
    cases.append(("groups_of_one_cell", x, np.arange(9), 9))
    cases.append(("one_group_is_the_population", x, np.zeros(9, dtype=np.int64), 1))
    cases.append(("groups_in_descending_row_order", x, np.asarray([2, 2, 2, 1, 1, 1, 0, 0, -1]), 3))
    cases.append(("float32", sp.csr_matrix(rng.normal(0, 1, (40, 5)).astype(np.float32) * (rng.random((40, 5)) < 0.5)),
                  rng.integers(0, 2, size=40), 2))
    cases.append(("one_window", rng.normal(0, 1, (70, 1)), rng.integers(0, 2, size=70), 2))
    cases.append(("one_cell", np.asarray([[0.5, 0.0, -1.0]]), np.asarray([0]), 1))
    cases.append(("one_cell_among_unlabelled", np.asarray([[0.5, 0.0], [1.0, 2.0], [3.0, -1.0]]), np.asarray([-1, 0, -1]), 1))
    # more windows than one LDS tile of the count and the scatter, and more rows than one slab
    many = np.round(rng.normal(0, 1, (SLAB + 9, TILE + 7)), 1) * (rng.random((SLAB + 9, TILE + 7)) < 0.004)
    many[:, TILE - 1:TILE + 1] = np.round(rng.normal(0, 1, (SLAB + 9, 2)), 1)  # the windows on both sides of the tile boundary
    many = sp.csr_matrix(many)
    code = rng.integers(-1, 3, size=SLAB + 9)
    cases.append(("two_window_tiles_csr", many, code, 3))
    cases.append(("two_window_tiles_dense", many.toarray(), code, 3))
    # a CSR row longer than one wavefront step, with an untested code among the tested
    wide = sp.csr_matrix(np.round(rng.normal(0, 1, (6, 200)), 1))
    cases.append(("rows_of_200_entries", wide, np.asarray([0, 1, 2, 0, 1, 2]), 2))
    return cases + lds_table_cases()

"""The written contract of tl.cnv_pseudobulk in numpy: np.rint, int64, np.add.at.

  1. stored values are used as float64 (a float32 is promoted exactly); an entry that is not stored is 0.
  2. shift e = min(40, 52 - bit_length(L_max)) for the largest kept group of L_max rows; every stored magnitude is
     < 2^10, so |q| < 2^50 and every sum stays below 2^62.
  3. q = rint(v 2^e), ties to even, as int64.
  4. S[g,w] = the int64 sum of q over the rows of the group, N[g,w] = the int32 number of stored values != 0.
  5. mean = (double(S) / double(L_g)) 2^-e, fraction = double(N) / double(L_g); L_g = 0 gives 0.

The kernel's two sizes are restated here (TILE, SLAB) because the edge cases are built around them.
"""
import fractions

import numpy as np
import scipy.sparse as sp

TILE = 4096       # windows per workgroup (csrc/icv_pseudobulk.hpp: kPbTile)
SLAB = 128        # listed rows per workgroup (kPbSlab)
MAX_SHIFT = 40
LIMIT = 1024.0


def shift_of(l_max):
    return min(MAX_SHIFT, 52 - int(l_max).bit_length())


def row_entries(x, r):
    """(columns, values) stored in row r of a CSR matrix as it stands (no sorting, no merging) or of a dense array."""
    if sp.issparse(x):
        a, b = int(x.indptr[r]), int(x.indptr[r + 1])
        return np.asarray(x.indices[a:b], dtype=np.int64), np.asarray(x.data[a:b])
    row = np.asarray(x[r])
    return np.arange(row.shape[0], dtype=np.int64), row


def quantise(v, shift):
    """Rule 3 for float64 values."""
    return np.rint(np.asarray(v, dtype=np.float64) * 2.0 ** shift).astype(np.int64)


def tables(x, rows, group_ptr, shift):
    """(S int64 G x W, N int32 G x W, flags) of rule 4 for lists of rows as the C ABI takes them: flags bit 0 for a
    non-finite value, bit 1 for a row number outside the matrix (skipped)."""
    if sp.issparse(x) and x.format != "csr":
        x = x.tocsr()
    n, w = x.shape
    g_count = len(group_ptr) - 1
    S = np.zeros((g_count, w), dtype=np.int64)
    N = np.zeros((g_count, w), dtype=np.int32)
    flags = 0
    for g in range(g_count):
        for r in rows[int(group_ptr[g]):int(group_ptr[g + 1])]:
            if not 0 <= r < n:
                flags |= 2
                continue
            cols, vals = row_entries(x, int(r))
            v = vals.astype(np.float64)
            if not np.isfinite(v).all():
                flags |= 1
            keep = (v != 0) & np.isfinite(v)
            np.add.at(S[g], cols[keep], quantise(v[keep], shift))
            np.add.at(N[g], cols[keep], 1)
    return S, N, flags


def finish(S, N, group_ptr, shift):
    """Rule 5."""
    L = np.diff(np.asarray(group_ptr, dtype=np.int64)).astype(np.float64)[:, None]
    mean = np.zeros(S.shape, dtype=np.float64)
    fraction = np.zeros(S.shape, dtype=np.float64)
    some = L[:, 0] > 0
    mean[some] = (S[some].astype(np.float64) / L[some]) * 2.0 ** -shift
    fraction[some] = N[some].astype(np.float64) / L[some]
    return mean, fraction


def lists(codes, n_groups):
    """(rows, group_ptr) of codes in [-1, n_groups): the rows of every group in ascending order, -1 in no list."""
    codes = np.asarray(codes, dtype=np.int64)
    rows = np.argsort(codes, kind="stable")[int((codes < 0).sum()):].astype(np.int64)
    group_ptr = np.zeros(n_groups + 1, dtype=np.int64)
    group_ptr[1:] = np.cumsum(np.bincount(codes[codes >= 0], minlength=n_groups))
    return rows, group_ptr


def profiles(x, codes, n_groups):
    """dict(mean, fraction, S, N, shift, n_cells) of the groups 0 .. n_groups - 1 of ``codes`` (all of them kept)."""
    rows, group_ptr = lists(codes, n_groups)
    n_cells = np.diff(group_ptr)
    shift = shift_of(int(n_cells.max()))
    S, N, _ = tables(x, rows, group_ptr, shift)
    mean, fraction = finish(S, N, group_ptr, shift)
    return {"mean": mean, "fraction": fraction, "S": S, "N": N, "shift": shift, "n_cells": n_cells, "rows": rows,
            "group_ptr": group_ptr}


def exact_mean(total, length, shift):
    """Rule 5 for one Python-int sum with ``fractions.Fraction``: float(total) rounds to nearest even, the quotient is
    rounded once, the scaling is exact."""
    return float(fractions.Fraction(float(int(total))) / int(length)) * 2.0 ** -shift


# ---- edge inputs: shared by the CPU test of this oracle and the GPU tests ------------------------------------------------------
def ties_case():
    """One row per group at shift 40: v 2^40 = k + 1/2 for even and odd k and both signs, next to the powers of two.
    dict(x dense float64, codes, want_q)."""
    ks = [0, 1, 2, 3, 4, 5, 2 ** 49 + 1, 2 ** 49 + 2, 2 ** 30, 2 ** 30 + 1]
    halves = [k + 0.5 for k in ks] + [-(k + 0.5) for k in ks]
    want = [int(round(h)) for h in halves]  # Python's round is ties-to-even
    vals = np.asarray(halves, dtype=np.float64) * 2.0 ** -40
    assert all(fractions.Fraction(float(v)) * 2 ** 40 == fractions.Fraction(h) for v, h in zip(vals, halves))
    x = np.zeros((1, len(halves)), dtype=np.float64)
    x[0] = vals
    return {"x": x, "codes": np.zeros(1, dtype=np.int64), "want_q": np.asarray(want, dtype=np.int64)}


def big_sum_case():
    """64 rows of values near 2^9 with low bits set: every S is about 2^55 and no multiple of 4, so it is no float64 and a
    float64 accumulator cannot hold it.  dict(x dense float64 64 x 7, codes, want_S as Python ints)."""
    rng = np.random.default_rng(11)
    q = (2 ** 49 + rng.integers(1, 2 ** 20, size=(64, 7))) | 1
    S = [int(sum(int(v) for v in q[:, j])) for j in range(7)]
    for j in range(7):  # (64 odd numbers: S is even; make S % 4 == 2)
        if S[j] % 4 == 0:
            q[1, j] += 2
            S[j] += 2
    x = q.astype(np.float64) * 2.0 ** -40
    assert all(int(v * 2.0 ** 40) == int(k) for v, k in zip(x.ravel(), q.ravel())) and (np.abs(x) < LIMIT).all()
    assert all(s > 2 ** 53 and s % 4 == 2 for s in S)
    return {"x": x, "codes": np.zeros(64, dtype=np.int64), "want_S": S}


def random_sparse(n, w, density, seed, dtype=np.float64):
    """A canonical CSR matrix of normal values with explicit stored 0.0 and -0.0 among the entries."""
    rng = np.random.default_rng(seed)
    dense = rng.normal(0.0, 0.5, (n, w)) * (rng.random((n, w)) < density)
    x = sp.csr_matrix(dense.astype(dtype))
    if x.nnz:
        pick = rng.choice(x.nnz, size=max(1, x.nnz // 20), replace=False)
        x.data[pick[::2]] = 0.0
        x.data[pick[1::2]] = -0.0
    return x


def planted_clones():
    """The recipe of DESIGN.md 4.17: 3 clones x 48 cells, 270 windows in 3 chromosomes, noise 0.5, a shift of 0.3 over
    145 windows.  dict(x dense float64, codes, truth int8 3 x 270, lengths)."""
    rng = np.random.default_rng(5)
    lengths = [120, 90, 60]
    truth = np.zeros((3, 270), dtype=np.int8)
    truth[0, 20:70] = 1
    truth[1, 130:190] = -1
    truth[1, 225:260] = 1
    codes = np.repeat(np.arange(3), 48)[rng.permutation(144)]
    x = rng.normal(0, 0.5, (144, 270)) + 0.3 * truth[codes]
    x[np.abs(x) < 0.15] = 0
    return {"x": x, "codes": codes, "truth": truth, "lengths": lengths}

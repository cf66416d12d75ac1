"""numpy oracle of tl.pca: float64 SVD of the (centred) dense matrix, sklearn 1.7's sign rule
(``svd_flip(u_based_decision=False)``), then the cast.  tests/test_pca_oracle.py pins it to the fixtures
recorded from sklearn; the GPU tests compare tl.pca with it.

For the two kernels on their own (tests/test_gpu_pca_edges.py): ``project_oracle`` restates icv_project's contract
with a correctly rounded fma in rational arithmetic, and ``integer_matrix`` / ``int_gram`` give inputs on which every
summation order of the Gram is exact."""
from __future__ import annotations

import glob
import os
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

PCA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pca")


def default_n_comps(n_obs, n_vars):
    """scanpy's default: 50, or min(n_obs, n_vars) - 1 when that is smaller."""
    return min(50, min(n_obs, n_vars) - 1)


def pca_oracle(X, n_comps, zero_center, dtype=np.float32):
    """(X_pca, components, explained_variance_ratio, explained_variance) as TruncatedSVD(algorithm="arpack")
    (zero_center=False) or PCA(svd_solver="arpack") (zero_center=True) define them."""
    X = X.toarray() if sp.issparse(X) else np.asarray(X)
    X = X.astype(np.float64)
    n = X.shape[0]
    Xc = X - X.mean(axis=0) if zero_center else X
    U, S, Vt = np.linalg.svd(Xc, full_matrices=False)
    U, S, Vt = U[:, :n_comps], S[:n_comps], Vt[:n_comps]
    signs = np.sign(Vt[np.arange(n_comps), np.argmax(np.abs(Vt), axis=1)])
    U, Vt = U * signs, Vt * signs[:, None]
    x_pca = U * S
    if zero_center:
        ev = S**2 / (n - 1)
        ratio = ev / np.var(X, ddof=1, axis=0).sum()
    else:
        ev = np.var(x_pca, axis=0)
        ratio = ev / np.var(X, axis=0).sum()
    return x_pca.astype(dtype), Vt, ratio, ev


def fixture_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(PCA_DIR, "pca_*.npz")))


def load_fixture(name):
    return dict(np.load(os.path.join(PCA_DIR, name + ".npz"), allow_pickle=False))


def ulp_tol(ref):
    """One float32 ulp of every column's largest |value|."""
    m = np.abs(ref).max(axis=0).astype(np.float32)
    return np.spacing(m).astype(np.float64)


# ---- icv_project: a float64 fma chain over the stored entries, one subtraction, one cast -----------------------------
def exact_fma(a, b, c):
    """The IEEE fma of three finite floats: a * b + c as a rational number, rounded once (Python's integer true
    division is correctly rounded)."""
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return r.numerator / r.denominator


def _rows(X):
    """(columns, values) of every row: a sparse matrix's stored entries in ascending column (stored zeros included), a
    dense row's non-zero elements in column order."""
    if sp.issparse(X):
        X = X.tocsr()
        if not X.has_sorted_indices:
            X = X.sorted_indices()
        for q in range(X.shape[0]):
            sl = slice(X.indptr[q], X.indptr[q + 1])
            yield X.indices[sl], X.data[sl]
    else:
        X = np.asarray(X)
        for row in X:
            cols = np.flatnonzero(row)  # -0.0 is a zero
            yield cols, row[cols]


def project_chain(X, V):
    """float64 ``n x k``: for every row and component, s = 0.0 and then s = fma(x, V[col, c], s) over the row's entries
    -- the part of project_oracle that costs (about 10 us per fma)."""
    V = np.asarray(V, dtype=np.float64)
    out = np.zeros((X.shape[0], V.shape[1]), dtype=np.float64)
    for q, (cols, vals) in enumerate(_rows(X)):
        xs = [float(x) for x in vals]
        for c in range(V.shape[1]):
            s = 0.0
            for x, v in zip(xs, V[cols, c].tolist()):
                s = exact_fma(x, v, s)
            out[q, c] = s
    return out


def project_oracle(X, V, shift=None, dtype=np.float64, chain=None):
    """icv_project's contract (csrc/icv_pca.hpp): the fma chain of project_chain, then ``s - shift[c]`` when a shift is
    given, then one cast to ``dtype``.  ``chain``: project_chain(X, V) computed before, to share it among calls."""
    s = project_chain(X, V) if chain is None else np.array(chain, dtype=np.float64)
    if shift is not None:
        s = s - np.asarray(shift, dtype=np.float64)[None, :]
    return s.astype(dtype)


def muladd_chain(X, V):
    """The chain a kernel without contraction would compute: s = s + x * v, two roundings per entry."""
    X = X.toarray() if sp.issparse(X) else np.asarray(X)
    X, V = X.astype(np.float64), np.asarray(V, dtype=np.float64)
    s = np.zeros((X.shape[0], V.shape[1]), dtype=np.float64)
    for j in range(X.shape[1]):
        s = s + X[:, j, None] * V[j][None, :]  # a zero element adds +-0.0: no change
    return s


def projection_case(n, w, k, seed, density=0.5, full_row=0, empty_row=1):
    """(X, V, shift): a dense float64 ``n x w`` matrix of values that are not float32 numbers, about ``density`` of
    them non-zero, with one full and one empty row (where n allows), and random ``w x k`` / ``k`` float64 V and shift."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, w)) * np.exp(rng.uniform(-3, 3, size=(1, w)))
    keep = rng.uniform(size=(n, w)) < density
    if full_row is not None and full_row < n:
        keep[full_row] = True
    x[~keep] = 0
    if empty_row is not None and empty_row < n:
        x[empty_row] = 0
    return x, rng.standard_normal((w, k)), rng.standard_normal(k)


# ---- icv_gram_f64: inputs on which X^T X is exact in any order --------------------------------------------------------
def integer_matrix(n, w, seed, density, lo=-7, hi=7, dtype=np.float32):
    """scipy CSR ``n x w`` of integers in [lo, hi] (zeros are not stored) at about ``density``, as ``dtype``.  Every
    partial sum of a Gram element is an integer below 2^53 in magnitude: float64 adds them exactly in any order."""
    m = max(abs(lo), abs(hi))
    assert n * m * m < 2 ** 53, "the Gram's partial sums must stay exact in float64"
    assert m < 2 ** 24, "the values must be float32 numbers"
    rng = np.random.RandomState(seed)
    flat = np.unique(rng.randint(0, n * w, size=int(round(density * n * w)), dtype=np.int64))
    vals = rng.randint(lo, hi + 1, size=flat.shape[0])
    flat, vals = flat[vals != 0], vals[vals != 0]
    return sp.csr_matrix((vals.astype(dtype), (flat // w, flat % w)), shape=(n, w))


def int_gram(X, dense=True):
    """X^T X of an integer-valued matrix in int64: a sparse product, made dense unless ``dense=False``."""
    X = sp.csr_matrix(X)
    Xi = X.astype(np.int64)
    assert (Xi != X).nnz == 0, "integer values only"
    m = int(np.abs(Xi.data).max()) if Xi.nnz else 0
    assert X.shape[0] * m * m < 2 ** 53
    G = (Xi.T @ Xi).tocsr()
    assert G.dtype == np.int64
    return G.toarray() if dense else G

"""Squared-distance matrices for the exact Ward tests (tests/test_ward_oracle.py, tests/test_gpu_ward_exact.py):
float32, symmetric, zero diagonal, full of ties.  They need not be Euclidean: the Ward entry point takes any matrix."""
from __future__ import annotations

import numpy as np

import _exact_inputs as E


def all_equal(n, value=1.0):
    """Every pair at the same distance: round 0 merges (0, 1), (2, 3), ... by the lowest-slot rule."""
    D = np.full((n, n), value, dtype=np.float32)
    np.fill_diagonal(D, 0)
    return D


def grid(n):
    """The first n points (row by row) of a regular 2-D integer grid ceil(sqrt(n)) wide."""
    w = int(np.ceil(np.sqrt(n)))
    p = np.stack(np.divmod(np.arange(n), w), axis=1).astype(np.int64)
    return ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1).astype(np.float32)


def valued(n, values, seed):
    """Independent draws from ``values`` above the diagonal, mirrored."""
    rng = np.random.default_rng(seed)
    D = np.triu(rng.choice(np.asarray(values, dtype=np.float32), size=(n, n)), 1)
    return (D + D.T).astype(np.float32)


def int_points(n, seed=None, d=3, lim=2):
    """(X, D): ``_exact_inputs.dist_case`` points on a small integer lattice (many duplicates and equal distances)
    and their exact squared distances as float32."""
    X, Zc = E.dist_case(n, d, seed=n if seed is None else seed, dup=n // 10, lim=lim)
    D = E.exact_sqdist(Zc)
    assert D.max(initial=0) < 2 ** 24
    return X, D.astype(np.float32)


def tie_matrix(name, n):
    return {"equal": lambda: all_equal(n), "grid": lambda: grid(n), "two": lambda: valued(n, [1, 2], n),
            "three": lambda: valued(n, [0, 1, 3], n + 1), "int": lambda: int_points(n)[1]}[name]()


TIE_KINDS = ("equal", "grid", "two", "three", "int")

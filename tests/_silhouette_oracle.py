"""The written contract of ``tl.cnv_silhouette`` in numpy, independent of the package.

``x`` is the n x C representation as float64 (a float32 value widens exactly), 1 <= C <= 256; ``codes`` gives the group
of every cell, -1 for a cell without a label: it is in no sum and its own width is NaN.  A group of no cells is skipped.

1. Distance.  From +0.0, over the components in ascending order: ``t = x_ic - x_jc``, ``acc = acc + t * t`` with the
   product rounded before the add (no fma); ``d_ij = sqrt(acc)``, correctly rounded.  ``d_ii`` is 0 and adds nothing;
   coincident cells count like any others.
2. Shift.  ``m`` = the largest ``|x|`` over all rows, ``L`` = the largest group size, ``b = math.frexp(m)[1]``,
   ``hc = (bit_length(C - 1) + 1) // 2``, ``e = min(40, 61 - bit_length(L) - (b + 1 + hc))`` and ``e = 40`` when
   ``m == 0``.  Since ``d < 2^(b + 1 + hc)`` every group sum stays below 2^62.  ``e < 0`` raises ``ValueError``, and so
   does a non-finite value.
3. Sums.  ``q_ij = rint(d_ij * 2^e)`` as int64, ties to even; ``S[i, g]`` = the int64 sum of ``q_ij`` over the j of g.
4. Means.  ``mean(i, g) = float64(S[i, g]) / (float64(cnt) * 2^e)``: the conversion rounds to nearest even, the divisor
   is exact, one correctly rounded division; ``cnt = n_g - 1`` for the cell's own group and ``n_g`` otherwise.
5. Width.  ``a`` = the own-group mean (0.0 where the own group is the cell alone), ``b`` = the smallest mean over the
   other non-empty groups, ``nearest`` = the lowest group that attains it; ``s = (b - a) / max(a, b)``, 0.0 where the own
   group has one cell and where ``max(a, b) == 0``.
6. Host.  The mean of a group is ``math.fsum(s of the group) / n_g`` (NaN for a group of no cells), the overall mean
   ``math.fsum`` over all labelled cells divided by their count.

Fewer than two non-empty groups raise ``ValueError``.
"""
from __future__ import annotations

import math

import numpy as np

MAX_SHIFT = 40
MAX_COMPONENTS = 256


def shift_of(m, largest_group, n_components):
    """Rule 2: (e, b + 1 + hc)."""
    hc = (int(n_components - 1).bit_length() + 1) // 2
    if m == 0:
        return MAX_SHIFT, 1 + hc
    dist_exp = math.frexp(m)[1] + 1 + hc
    return min(MAX_SHIFT, 61 - int(largest_group).bit_length() - dist_exp), dist_exp


def distances(x):
    """Rule 1 for all pairs: the n x n float64 matrix."""
    n, c = x.shape
    acc = np.zeros((n, n), dtype=np.float64)
    for k in range(c):
        t = x[:, k][:, None] - x[:, k][None, :]
        acc = acc + t * t
    return np.sqrt(acc)


def silhouette(x, codes, n_groups=None):
    """dict of ``s``, ``a``, ``b`` (float64 n, NaN without a label), ``nearest`` (int32 n, -1 without a label),
    ``shift``, ``S`` (int64 n x G, rows of unlabelled cells 0), ``sizes`` (int64 G), ``mean`` and ``group_mean``
    (float64 G)."""
    x = np.asarray(x, dtype=np.float64)
    codes = np.asarray(codes, dtype=np.int64)
    n, c = x.shape
    if not 1 <= c <= MAX_COMPONENTS:
        raise ValueError("1 <= C <= 256")
    if not np.isfinite(x).all():
        raise ValueError("non-finite values")
    g = int(codes.max(initial=-1)) + 1 if n_groups is None else int(n_groups)
    sizes = np.bincount(codes[codes >= 0], minlength=g).astype(np.int64)
    if np.count_nonzero(sizes) < 2:
        raise ValueError("fewer than two non-empty groups")
    m = float(np.abs(x).max()) if x.size else 0.0
    e, _ = shift_of(m, int(sizes.max()), c)
    if e < 0:
        raise ValueError("e < 0")
    scale = 2.0 ** e

    q = np.rint(distances(x) * scale).astype(np.int64)
    S = np.zeros((n, g), dtype=np.int64)
    for k in range(g):
        S[:, k] = q[:, codes == k].sum(axis=1, dtype=np.int64)
    S[codes < 0] = 0

    s = np.full(n, np.nan)
    a = np.full(n, np.nan)
    b = np.full(n, np.nan)
    nearest = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        own = int(codes[i])
        if own < 0:
            continue
        ai, bi, at = 0.0, 0.0, -1
        for k in range(g):
            cnt = int(sizes[k]) - 1 if k == own else int(sizes[k])
            if cnt <= 0:
                continue
            mean = float(np.float64(S[i, k]).item()) / (float(cnt) * scale)
            if k == own:
                ai = mean
            elif at < 0 or mean < bi:
                bi, at = mean, k
        top = max(ai, bi)
        s[i] = 0.0 if sizes[own] <= 1 or top == 0.0 else (bi - ai) / top
        a[i], b[i], nearest[i] = ai, bi, at
    group_mean = np.array([math.fsum(s[codes == k].tolist()) / int(sizes[k]) if sizes[k] else np.nan for k in range(g)])
    labelled = codes >= 0
    mean = math.fsum(s[labelled].tolist()) / int(np.count_nonzero(labelled))
    return {"s": s, "a": a, "b": b, "nearest": nearest, "shift": e, "S": S, "sizes": sizes, "mean": mean,
            "group_mean": group_mean}


def brute_force(x, codes):
    """(s, a, b) by ``scipy.spatial.distance.cdist`` and ``math.fsum``: no quantisation, for the derived tolerance."""
    from scipy.spatial.distance import cdist

    x = np.asarray(x, dtype=np.float64)
    codes = np.asarray(codes, dtype=np.int64)
    d = cdist(x, x)
    n = x.shape[0]
    g = int(codes.max()) + 1
    sizes = np.bincount(codes[codes >= 0], minlength=g)
    s, a, b = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        own = int(codes[i])
        if own < 0:
            continue
        means = {}
        for k in range(g):
            cnt = sizes[k] - 1 if k == own else sizes[k]
            if cnt > 0:
                members = np.flatnonzero(codes == k)
                means[k] = math.fsum(d[i, members[members != i]].tolist()) / cnt
        ai = means.get(own, 0.0)
        bi = min(v for k, v in means.items() if k != own)
        top = max(ai, bi)
        s[i] = 0.0 if sizes[own] <= 1 or top == 0.0 else (bi - ai) / top
        a[i], b[i] = ai, bi
    return s, a, b


def planted(seed):
    """The planted case of the issue: (x float32 125 x 10, true labels)."""
    true = np.repeat([0, 1, 2], [60, 40, 25])
    cen = np.zeros((3, 10))
    cen[np.arange(3), np.arange(3)] = 2.0
    x = (cen[true] + np.random.default_rng(seed).normal(0, 0.5, (125, 10))).astype(np.float32)
    return x, true

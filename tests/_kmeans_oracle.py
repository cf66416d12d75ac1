"""The written contract of ``tl.cnv_kmeans`` in numpy, independent of the package.

``x`` is the n x C representation as float64 (a float32 value widens exactly), 1 <= C <= 256; 2 <= k <= 256, k <= n.

1. Squared distance.  From +0.0, over the components in ascending order: ``t = x_ic - c_gc``, ``acc = acc + t * t`` with
   the product rounded before the add (no fma); ``D(i, g) = acc``.  No square root here.
2. Shifts.  ``m`` = the largest ``|value|`` of the representation and of a given ``init`` array, ``b = frexp(m)[1]``,
   ``e = min(40, 62 - bit_length(n) - b)`` (coordinates: ``|rint(x 2^e)| <= 2^(b + e)``, so a sum over n cells stays
   within int64) and ``f = min(40, 61 - bit_length(n) - (2b + 2 + bit_length(C - 1)))`` (squared distances:
   ``D < 2^(2b + 2 + bit_length(C - 1))``); both 40 when ``m == 0``.  ``e < 0``, ``f < 0`` and a non-finite value raise
   ``ValueError``.
3. Hash.  ``mix`` is the splitmix64 finaliser; ``base_r = mix(((random_state + r) mod 2^64) ^ mix(TAG))`` for run r and
   ``z_t = mix(base_r ^ t)``.
4. Seeding (k-means++, one candidate per draw).  Centre 0 is row ``z_0 mod n``.  For t = 1 .. k - 1:
   ``w_i = rint(min_{g < t} D(i, g) 2^f)`` as int64, ties to even; ``P`` the inclusive prefix sum of ``w`` in row order,
   ``W = P_{n-1}``, ``theta = z_t mod W``; centre t is the first row i with ``P_i > theta``.  ``W == 0`` raises
   ``ValueError``.
5. Assignment.  ``label_i`` is the lowest g that attains ``min_g D(i, g)``; ``n_changed`` counts the labels that differ
   from the previous iteration's (all n in iteration 1); the inertia is ``I = sum_i rint(D(i, label_i) 2^f)``, int64.
6. Update.  ``q_ic = rint(x_ic 2^e)`` as int64; ``Q[g, c]`` = the int64 sum of ``q_ic`` over the cells of g;
   ``c_gc = float64(Q[g, c]) / (float64(n_g) 2^e)``: one conversion to nearest even, an exact divisor, one correctly
   rounded division.  A cluster without cells keeps its centre.
7. Loop.  Iteration ``it`` assigns against the current centres; ``n_changed == 0`` stops with ``converged=True``;
   otherwise ``it == max_iter`` stops with ``converged=False``; otherwise update and go on.  The returned labels are the
   last assignment, the returned centres the ones they were assigned against.
8. Restarts.  Runs r = 0 .. n_init - 1; the lowest integer inertia wins, ties to the lowest r; the returned inertia is
   ``float64(I) 2^-f``.
9. Renumbering.  The largest cluster comes first, ties in size go to the lower raw index, so clusters without cells
   come last.
"""
from __future__ import annotations

import math

import numpy as np

from _silhouette_oracle import planted  # noqa: F401  (the planted case is shared)

MAX_SHIFT = 40
MAX_COMPONENTS = 256
MAX_CLUSTERS = 256
TAG = 0x6B6D65616E73  # "kmeans"
_MASK = (1 << 64) - 1


def mix(z):
    z &= _MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK
    return z ^ (z >> 31)


def run_base(random_state, r):
    return mix(((int(random_state) + r) & _MASK) ^ mix(TAG))


def shifts(m, n, n_components):
    """Rule 2: (e, f)."""
    if m == 0:
        return MAX_SHIFT, MAX_SHIFT
    b = math.frexp(m)[1]
    nb = int(n).bit_length()
    return (min(MAX_SHIFT, 62 - nb - b),
            min(MAX_SHIFT, 61 - nb - (2 * b + 2 + int(n_components - 1).bit_length())))


def sqdist(x, centres):
    """Rule 1: the n x k float64 matrix D."""
    acc = np.zeros((x.shape[0], centres.shape[0]), dtype=np.float64)
    for c in range(x.shape[1]):
        t = x[:, c][:, None] - centres[:, c][None, :]
        acc = acc + t * t
    return acc


def seed_rows(x, k, f, base):
    """Rule 4: the k seeded rows, in raw order."""
    n = x.shape[0]
    picks = [mix(base ^ 0) % n]
    mind = None
    for t in range(1, k):
        d = sqdist(x, x[picks[-1]][None, :])[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
        w = np.rint(mind * 2.0 ** f).astype(np.int64)
        p = np.cumsum(w, dtype=np.int64)
        total = int(p[-1])
        if total == 0:
            raise ValueError(f"fewer than {t + 1} distinct points")
        theta = mix(base ^ t) % total
        picks.append(int(np.searchsorted(p, theta, side="right")))  # the first i with P_i > theta
    return picks


def lloyd(x, centres, e, f, max_iter):
    """Rules 5-7 from the given centres: (labels int32, centres, D of the labels, I, n_iter, converged, history)."""
    n, k = x.shape[0], centres.shape[0]
    centres = centres.copy()
    q = np.rint(x * 2.0 ** e).astype(np.int64)
    prev = np.full(n, -1, dtype=np.int64)
    history = []
    it = 0
    while True:
        it += 1
        d = sqdist(x, centres)
        labels = np.argmin(d, axis=1)  # the first index that attains the minimum
        dmin = d[np.arange(n), labels]
        inertia = int(np.rint(dmin * 2.0 ** f).astype(np.int64).sum(dtype=np.int64))
        changed = int(np.count_nonzero(labels != prev))
        history.append((inertia, changed))
        if changed == 0:
            converged = True
            break
        if it == max_iter:
            converged = False
            break
        for g in range(k):
            members = labels == g
            n_g = int(np.count_nonzero(members))
            if n_g:
                total = q[members].sum(axis=0, dtype=np.int64)
                centres[g] = total.astype(np.float64) / (float(n_g) * 2.0 ** e)
        prev = labels
    return labels.astype(np.int32), centres, dmin, inertia, it, converged, history


def renumber(labels, k):
    """Rule 9: (order, sizes in the new order): ``order[j]`` is the raw index of the new cluster j."""
    sizes = np.bincount(labels, minlength=k).astype(np.int64)
    order = np.argsort(-sizes, kind="stable")
    return order, sizes[order]


def kmeans(x, k, random_state=0, n_init=10, max_iter=300, init=None):
    """dict of ``labels`` (int32, renumbered), ``centers`` (k x C, renumbered), ``sqdist`` and ``distance`` (float64 n),
    ``sizes``, ``inertia_q`` (int, the winner's), ``inertia``, ``n_iter``, ``converged``, ``shift``, ``best_init``, and per
    run ``history``, ``picks`` (None with a given ``init``) and ``inertia_all``."""
    x = np.asarray(x, dtype=np.float64)
    n, c = x.shape
    if not 1 <= c <= MAX_COMPONENTS:
        raise ValueError("1 <= C <= 256")
    if not (2 <= k <= MAX_CLUSTERS and k <= n):
        raise ValueError("2 <= k <= min(256, n)")
    if not np.isfinite(x).all():
        raise ValueError("non-finite values")
    m = float(np.abs(x).max())
    if init is not None:
        init = np.asarray(init, dtype=np.float64)
        if init.shape != (k, c):
            raise ValueError("init must be k x C")
        if not np.isfinite(init).all():
            raise ValueError("non-finite values in init")
        m = max(m, float(np.abs(init).max()))
        n_init = 1
    e, f = shifts(m, n, c)
    if e < 0 or f < 0:
        raise ValueError("rescale")
    runs, all_picks = [], []
    for r in range(n_init):
        if init is None:
            picks = seed_rows(x, k, f, run_base(random_state, r))
            start = x[picks]
        else:
            picks, start = None, init
        all_picks.append(picks)
        runs.append(lloyd(x, start, e, f, max_iter))
    inertia_all = [run[3] for run in runs]
    best = int(np.argmin(inertia_all))  # the first run that attains the minimum
    labels, centres, dmin, inertia, n_iter, converged, _ = runs[best]
    order, sizes = renumber(labels, k)
    new_of_raw = np.empty(k, dtype=np.int32)
    new_of_raw[order] = np.arange(k, dtype=np.int32)
    return {"labels": new_of_raw[labels], "centers": centres[order], "sqdist": dmin, "distance": np.sqrt(dmin),
            "sizes": sizes, "inertia_q": inertia, "inertia": float(inertia) * 2.0 ** -f, "n_iter": n_iter,
            "converged": converged, "shift": (e, f), "best_init": best, "history": [run[6] for run in runs],
            "picks": all_picks, "inertia_all": inertia_all}


def blobs(seed):
    """(x float32 2000 x 20, true labels): 8 centres ``normal(0, 3)``, labels ``integers(0, 8, 2000)``, noise 1."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0, 3, (8, 20))
    true = rng.integers(0, 8, 2000)
    x = (centres[true] + rng.normal(0, 1, (2000, 20))).astype(np.float32)
    return x, true

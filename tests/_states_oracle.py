"""Numpy / pure-Python oracle of tl.cnv_states, and the builders of its test cases.

The rules, implemented literally with Python floats (IEEE float64, no fused multiply-add), explicit loops over the
windows and ``math.fsum``:

1. Parameters.  ``sigma=None``: ``sqrt(S / (n W))``, ``S = fsum(q_i)``, ``q_i`` = the sum of ``v v`` over row i's stored
   entries in stored order (ascending column of the canonical CSR), one sequential float64 sum per row.  ``sigma == 0``
   gives all-neutral output.  ``amplitude=None``: ``2 sigma``.  ``h = 1.0 / (2.0 sigma sigma)``,
   ``stay = log(1 - p)``, ``sw = log(p / 2)``.
2. Emission of state s in {0, 1, 2} with means (-a, 0.0, +a): ``t = x - mu_s``, ``e_s = -(t t) h``.
3. Chain over the windows of one chromosome: ``d_0(s) = e_s(x_0)``;
   ``d_t(s) = best_r(d_{t-1}(r) + T(r, s)) + e_s(x_t)`` with ``T = stay`` for r = s and ``sw`` otherwise; ``best`` takes
   the largest value, ties go to r = s first, then to the lower r.
4. The last window takes the s with the largest d; ties go to neutral, then loss, then gain.  Then backtrack.
5. Output = state - 1.  An entry that is not stored is 0.0; chains never cross a chromosome boundary.
6. Overflow: with ``m`` the largest ``|v|`` over the stored values and ``t = m + a``, a ``(t t) h`` that is not finite is
   a ``ValueError``: the state ``-a`` sees that ``t`` for a positive value and the state ``+a`` for a negative one, and
   every other emission is smaller in magnitude, so all emissions are finite exactly when this one is.

``bounds=`` takes the kernel's own ``chr_start`` array (C + 1 ascending window numbers inside [0, W]) in place of
``chr_pos``: a chromosome with ``s1 <= s0`` is skipped, a window that no chromosome covers stays neutral.
"""
import fractions
import functools
import math
import random

import numpy as np
import scipy.sparse as sp

MAX_WINDOWS = 16384  # ICV_STATES_MAX_WINDOWS of include/infercnv_hip.h
END_ORDER = (1, 0, 2)  # rule 4: neutral, then loss, then gain


# ---- rule 1 --------------------------------------------------------------------------------------------------------------
def canonical(x):
    """Canonical float64 CSR (ascending unique columns) of a scipy sparse matrix or a dense array; a dense array
    stores every element."""
    if sp.issparse(x):
        x = x.tocsr().astype(np.float64)
        if not x.has_canonical_format:
            x = x.copy()
            x.sum_duplicates()
        return x
    a = np.asarray(x, dtype=np.float64)
    n, w = a.shape
    return sp.csr_matrix((a.ravel().copy(), np.tile(np.arange(w, dtype=np.int32), n), np.arange(n + 1) * w),
                         shape=(n, w))


def rowsq(x):
    """q_i of rule 1: list of n Python floats."""
    x = canonical(x)
    data, indptr = x.data.tolist(), x.indptr.tolist()
    out = []
    for i in range(x.shape[0]):
        s = 0.0
        for k in range(indptr[i], indptr[i + 1]):
            v = data[k]
            s = s + v * v
        out.append(s)
    return out


def default_sigma(x):
    n, w = x.shape
    return math.sqrt(math.fsum(rowsq(x)) / (float(n) * float(w)))


def scalars(sigma, switch_prob):
    """(h, stay, sw) of rule 1."""
    return 1.0 / (2.0 * sigma * sigma), math.log(1.0 - switch_prob), math.log(switch_prob / 2.0)


def bounds(chr_pos, n_windows):
    starts = sorted(int(v) for v in chr_pos.values())
    return starts + [int(n_windows)]


_bounds_of = bounds  # (cnv_states has a keyword of that name)


def check_emissions(x, amplitude, sigma, who="cnv_states"):
    """rule 6 on a canonical CSR matrix."""
    m = max((abs(v) for v in x.data.tolist()), default=0.0)
    h = 1.0 / (2.0 * sigma * sigma)
    t = m + amplitude
    if not math.isfinite((t * t) * h):
        raise ValueError(f"{who}: sigma={sigma!r} and amplitude={amplitude!r} overflow the emission of the value of "
                         f"magnitude {m!r}")


def overflow_case():
    """(x, chr_pos, kwargs): one stored value of 1e160 under sigma = 0.1, amplitude = 0.2, where every emission of its
    window is -inf."""
    x = sp.csr_matrix(np.array([[0.0, 0.3, 1e160, -0.2, 0.0, 0.1]]))
    return x, {"chr1": 0}, {"sigma": 0.1, "amplitude": 0.2}


def largest_value_that_does_not_overflow(amplitude, sigma):
    """The largest float64 m with ((m + a) (m + a)) h finite, by bisection on rule 6 itself."""
    h = 1.0 / (2.0 * sigma * sigma)

    def ok(m):
        t = m + amplitude
        return math.isfinite((t * t) * h)

    lo, hi = 1.0, 1e160
    assert ok(lo) and not ok(hi)
    while math.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2.0
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


# ---- rules 2-4 -----------------------------------------------------------------------------------------------------------
def emissions(x, a, h):
    """rule 2: (e_0, e_1, e_2) of one value."""
    out = []
    for mu in (-a, 0.0, a):
        t = x - mu
        out.append(-(t * t) * h)
    return out


def transition(r, s, stay, sw):
    return stay if r == s else sw


VARIANTS = ("assoc", "emul", "fma")  # deviations from rules 2-3 that a compiler or a rewrite could introduce


def _emissions_emul(x, a, h):
    """not rule 2: -(t (t h))."""
    out = []
    for mu in (-a, 0.0, a):
        t = x - mu
        out.append(-(t * (t * h)))
    return out


def _fma_add(best, x, mu, h):
    """not rule 3: best + e with the product -(t t) h left unrounded (one fused multiply-add), exactly."""
    t = x - mu
    return float(fractions.Fraction(best) - fractions.Fraction(t * t) * fractions.Fraction(h))


def viterbi_chain(xs, a, h, stay, sw, variant=None):
    """rules 3-4 on the values of one chromosome: the list of states (0 loss, 1 neutral, 2 gain).

    ``variant`` names a deviation that the tests show to be visible (never the contract): ``"assoc"`` adds
    ``d(r) + (T + e)``, ``"emul"`` forms ``-(t (t h))``, ``"fma"`` fuses the product ``-(t t) h`` into the add."""
    assert variant is None or variant in VARIANTS
    emit = _emissions_emul if variant == "emul" else emissions
    mus = (-a, 0.0, a)
    d = emit(xs[0], a, h)
    back = []
    for x in xs[1:]:
        e = emit(x, a, h)
        nd, arg = [], []
        for s in range(3):
            if variant == "assoc":
                best, who = d[s] + (stay + e[s]), s
                for r in range(3):
                    if r == s:
                        continue
                    cand = d[r] + (sw + e[s])
                    if cand > best:
                        best, who = cand, r
                nd.append(best)
                arg.append(who)
                continue
            best, who = d[s] + stay, s  # r = s first
            for r in range(3):  # then the others, the lower r first; only a strictly larger value replaces
                if r == s:
                    continue
                cand = d[r] + sw
                if cand > best:
                    best, who = cand, r
            nd.append(_fma_add(best, x, mus[s], h) if variant == "fma" else best + e[s])
            arg.append(who)
        d = nd
        back.append(arg)
    s = END_ORDER[0]
    for c in END_ORDER[1:]:
        if d[c] > d[s]:
            s = c
    path = [s]
    for arg in reversed(back):
        s = arg[s]
        path.append(s)
    path.reverse()
    return path


def path_score(xs, path, a, h, stay, sw):
    """The log-score of one path, summed in the order of rule 3: ((previous + T) + e)."""
    sc = emissions(xs[0], a, h)[path[0]]
    for t in range(1, len(xs)):
        sc = (sc + transition(path[t - 1], path[t], stay, sw)) + emissions(xs[t], a, h)[path[t]]
    return sc


# ---- the whole function ----------------------------------------------------------------------------------------------------
def cnv_states(x, chr_pos, amplitude=None, sigma=None, switch_prob=1e-3, bounds=None):
    """(states int8 n x W, fraction float64 n, params dict) of rules 1-6."""
    x = canonical(x)
    n, w = x.shape
    if sigma is None:
        sigma = default_sigma(x)
    if amplitude is None:
        amplitude = 2.0 * sigma
    params = {"amplitude": float(amplitude), "sigma": float(sigma), "switch_prob": float(switch_prob)}
    out = np.zeros((n, w), dtype=np.int8)
    if sigma == 0.0:
        return out, np.zeros(n, dtype=np.float64), params
    h, stay, sw = scalars(float(sigma), float(switch_prob))
    a = float(amplitude)
    check_emissions(x, a, float(sigma))
    edges = [int(v) for v in bounds] if bounds is not None else _bounds_of(chr_pos, w)
    data, indices, indptr = x.data.tolist(), x.indices.tolist(), x.indptr.tolist()
    for i in range(n):
        row = [0.0] * w
        for k in range(indptr[i], indptr[i + 1]):
            row[indices[k]] = data[k]
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 > s0:
                out[i, s0:s1] = np.asarray(viterbi_chain(row[s0:s1], a, h, stay, sw), dtype=np.int8) - 1
    count = (out != 0).sum(axis=1)
    return out, count.astype(np.float64) / float(w), params


# ---- case builders ---------------------------------------------------------------------------------------------------------
def chr_pos_of(lengths):
    """{"chr1": 0, "chr2": len_1, ...}, inserted in shuffled order (the function sorts by start, not by name)."""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()
    order = list(range(len(lengths)))
    order = order[1::2] + order[0::2]
    return {f"chr{c + 1}": int(starts[c]) for c in order}


def planted(n, chrom_lengths, seed, s=0.1, keep=1.5):
    """A CNV-like matrix with a known truth: noise N(0, s); in every chromosome of at least 5 windows, with probability
    1/2, one segment of 5 .. 15 windows shifted by +6 s or -6 s; values with |v| < keep s dropped (not stored).
    dict(x=canonical CSR float64, chr_pos, truth=int8 n x W, kwargs={})."""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in chrom_lengths]
    w = int(sum(lengths))
    dense = rng.normal(0.0, s, size=(n, w))
    truth = np.zeros((n, w), dtype=np.int8)
    start = 0
    for length in lengths:
        if length >= 5:
            plant = rng.random(n) < 0.5
            seg = rng.integers(5, min(length, 15) + 1, size=n)
            off = np.floor(rng.random(n) * (length - seg + 1)).astype(np.int64)
            sign = np.where(rng.random(n) < 0.5, -1, 1)
            for i in np.flatnonzero(plant):
                a, b = start + off[i], start + off[i] + seg[i]
                dense[i, a:b] += sign[i] * 6.0 * s
                truth[i, a:b] = sign[i]
        start += length
    dense[np.abs(dense) < keep * s] = 0.0
    return {"x": sp.csr_matrix(dense), "chr_pos": chr_pos_of(lengths), "truth": truth, "kwargs": {}}


TIES_LENGTHS = (7, 5, 1, 3, 6, 2)
TIES_A = 0.5  # a power of two; sigma = 0.25 makes h = 8.0: every emission is exact
TIES_KWARGS = {"amplitude": TIES_A, "sigma": 0.25, "switch_prob": 1e-3}


def ties():
    """Rows whose entries are exactly 0, +-a/2 (two states emit the same) and +-a, with a power-of-two amplitude: rows of
    one repeated value, alternating and mirrored rows, seeded draws from the five values, an all-zero row (nothing
    stored) and a row in which every window is stored (zeros included).  Explicit zeros stay stored entries."""
    a = TIES_A
    w = sum(TIES_LENGTHS)
    vals = np.array([0.0, a / 2, -a / 2, a, -a])
    rows = [np.full(w, v) for v in vals]
    rows += [np.where(np.arange(w) % 2 == 0, u, v) for u in vals for v in vals if u != v]
    rng = np.random.default_rng(7)
    rows += [vals[rng.integers(0, 5, size=w)] for _ in range(12)]
    rows += [vals[rng.integers(0, 3, size=w)] for _ in range(6)]
    stored = [np.ones(w, dtype=bool) if i % 3 == 0 else (r != 0.0) | (rng.random(w) < 0.3) for i, r in enumerate(rows)]
    rows.append(np.zeros(w))
    stored.append(np.zeros(w, dtype=bool))  # the all-zero row: no stored entry
    rows.append(vals[rng.integers(0, 5, size=w)])
    stored.append(np.ones(w, dtype=bool))  # every window stored
    data, indices, indptr = [], [], [0]
    for r, m in zip(rows, stored):
        m = m | (r != 0.0)
        cols = np.flatnonzero(m)
        data.extend(r[cols].tolist())
        indices.extend(cols.tolist())
        indptr.append(len(data))
    x = sp.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32),
                       np.asarray(indptr, dtype=np.int64)), shape=(len(rows), w))
    return {"x": x, "chr_pos": chr_pos_of(TIES_LENGTHS), "kwargs": dict(TIES_KWARGS)}


ROUNDING_LENGTHS = (2, 3, 6)
ROUNDING_CHAINS = 400  # per length
ROUNDING_ROWS = 4
ROUNDING_SEED = 1
ROUNDING_KWARGS = {"amplitude": 0.23, "sigma": 0.1, "switch_prob": 1e-3}  # nothing dyadic: every operation rounds


def rounding_ties(seed=ROUNDING_SEED):
    """Chains in which the last bit of the sums decides the call.  A chain of L windows has L - 1 values
    ``a / 2 + N(0, sigma / 2)`` and a last value of ``L a / 2`` minus their sum: in exact arithmetic the all-neutral and
    the all-gain path score the same.  400 chains of each L in (2, 3, 6), 100 of each per row (300 chromosomes a row:
    the lanes take several each); the odd rows are mirrored (-x), where loss takes the place of gain.
    dict(x, chr_pos, kwargs, chains={L: [(row, first window)]})."""
    rng = random.Random(seed)
    a, sigma = ROUNDING_KWARGS["amplitude"], ROUNDING_KWARGS["sigma"]
    per_row = ROUNDING_CHAINS // ROUNDING_ROWS
    lengths = [L for L in ROUNDING_LENGTHS for _ in range(per_row)]
    w = sum(lengths)
    dense = np.zeros((ROUNDING_ROWS, w))
    chains = {L: [] for L in ROUNDING_LENGTHS}
    for i in range(ROUNDING_ROWS):
        t = 0
        for L in lengths:
            xs = [a / 2 + rng.gauss(0.0, sigma / 2) for _ in range(L - 1)]
            xs.append(L * a / 2 - sum(xs))
            dense[i, t:t + L] = xs
            chains[L].append((i, t))
            t += L
    dense[1::2] *= -1.0
    return {"x": canonical(dense), "chr_pos": chr_pos_of(lengths), "kwargs": dict(ROUNDING_KWARGS), "chains": chains}


def rounding_differences(c, variant):
    """{L: the number of the case's chains of L windows whose calls under ``variant`` are not the contract's}."""
    dense = c["x"].toarray()
    kw = c["kwargs"]
    h, stay, sw = scalars(kw["sigma"], kw["switch_prob"])
    out = {}
    for L, where in c["chains"].items():
        n = 0
        for i, t in where:
            xs = dense[i, t:t + L].tolist()
            n += viterbi_chain(xs, kw["amplitude"], h, stay, sw) != viterbi_chain(xs, kw["amplitude"], h, stay, sw, variant)
        out[L] = n
    return out


SPLIT_WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65)
SPLIT_ROWS = 9
SPLIT_KWARGS = {"amplitude": TIES_A, "sigma": 0.25, "switch_prob": 0.3}


def output_split(w):
    """9 rows of w windows from {0, +a, -a}, the first and the last window never 0, under switch_prob = 0.3 (one switch
    costs 1.54, a window on a state's mean is worth 2 over neutral): most calls are not 0, and rows follow each other
    w bytes apart, so the int8 row's single-byte head, its 4-byte words and its tail take every split.
    dict(x, chr_pos, kwargs)."""
    rng = np.random.default_rng(1000 + w)
    a = SPLIT_KWARGS["amplitude"]
    dense = rng.choice([0.0, a, -a], size=(SPLIT_ROWS, w), p=[0.2, 0.4, 0.4])
    dense[:, 0] = np.where(rng.random(SPLIT_ROWS) < 0.5, a, -a)
    dense[:, -1] = np.where(rng.random(SPLIT_ROWS) < 0.5, a, -a) if w > 1 else dense[:, 0]
    lengths = [w] if w < 6 else [w // 2, 1, w - w // 2 - 1]
    return {"x": canonical(dense), "chr_pos": chr_pos_of(lengths), "kwargs": dict(SPLIT_KWARGS)}


def shapes():
    """Chromosome layouts at which the kernel takes another path: {name: case}."""
    rng = np.random.default_rng(11)
    many65 = rng.integers(1, 7, size=65).tolist()
    many130 = rng.integers(1, 7, size=130).tolist()
    out = {
        "single_chromosome": planted(5, [50], 1),
        "one_window": planted(3, [1], 2, keep=0.5),
        "one_window_chromosome_between_long": planted(9, [30, 1, 30], 3),
        "chromosomes_65": planted(7, many65, 4),
        "chromosomes_130": planted(6, many130, 5),
        "max_windows": planted(2, [9000, 7000, MAX_WINDOWS - 16000], 6),
    }
    return out


def full_and_empty():
    """The longest row has all W entries stored, next to rows without any."""
    base = planted(6, [100, 1, 199], 8)
    dense = base["x"].toarray()
    rng = np.random.default_rng(9)
    dense[0] = 0.0
    dense[1] = rng.normal(0.0, 0.1, size=dense.shape[1])
    dense[1][dense[1] == 0.0] = 0.05
    dense[2] = 0.0
    dense[5] = 0.0
    base["x"] = sp.csr_matrix(dense)
    return base


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its expected output, computed once: dict(x, chr_pos, kwargs, states, fraction, params)."""
    if name == "ties":
        c = ties()
    elif name == "rounding_ties":
        c = rounding_ties()
    elif name.startswith("output_split_"):
        c = output_split(int(name[len("output_split_"):]))
    elif name == "planted777":
        c = planted(777, [40, 1, 25, 60], 0)
    elif name == "full_and_empty":
        c = full_and_empty()
    else:
        c = shapes()[name]
    c["states"], c["fraction"], c["params"] = cnv_states(c["x"], c["chr_pos"], **c["kwargs"])
    for v in (c["states"], c["fraction"]):
        v.setflags(write=False)
    return c


SHAPE_NAMES = ("single_chromosome", "one_window", "one_window_chromosome_between_long", "chromosomes_65",
               "chromosomes_130", "max_windows")

"""Numpy / pure-Python oracle of tl.cnv_copy_states, and the builders of its test cases.

The rules, implemented literally with Python floats (IEEE float64, no fused multiply-add) and explicit loops over the
windows and the K states:

1. Parameters.  ``levels``: K finite floats, 2 <= K <= 8, strictly ascending, exactly one of them 0.0 (the neutral state,
   at index z; ``-0.0`` is used as ``0.0``).  ``levels=None``: ``[float(k) * amplitude for k in (-2, -1, 0, 1, 2, 3)]``.
   ``sigma`` and ``amplitude`` default as in ``_states_oracle`` (the RMS of the matrix, ``2 sigma``); ``sigma == 0`` gives
   all-neutral output.  ``h = 1.0 / (2.0 sigma sigma)``, ``stay = log(1 - p)``, ``sw = log(p / (K - 1))``.
2. Emission of state s: ``t = x - mu_s``, ``e_s = -(t t) h``.  An entry that is not stored is 0.0.
3. Chain over the windows of one chromosome: ``d_0(s) = e_s(x_0)``;
   ``d_t(s) = best_r(d_{t-1}(r) + T(r, s)) + e_s(x_t)`` with ``T = stay`` for r = s and ``sw`` otherwise; ``best`` takes
   the largest value, ties go to r = s first, then to the lowest r: only a strictly larger value replaces.
4. The last window takes the s with the largest d, the states tried in the order z, z - 1, z + 1, z - 2, z + 2, ...
   (those that exist); only a strictly larger value replaces.  Then backtrack.
5. Output = s - z as int8; chains never cross a chromosome boundary; a window that no chromosome covers is 0.
6. Overflow: with ``m`` the largest ``|v|`` over the stored values and ``t = m + max(|levels[0]|, |levels[K-1]|)``, a
   ``(t t) h`` that is not finite is a ``ValueError``.

Rule 3 is the K^2 form here, whatever the kernel does; ``viterbi_chain_two_best`` restates the kernel's O(K) form and
its named mistakes, to show on the CPU which cases tell them from the contract.  ``bounds=`` takes the kernel's own ``chr_start`` array in place
of ``chr_pos``, as in ``_states_oracle``.
"""
import fractions
import functools
import math
import random

import numpy as np

import _states_oracle as so

MAX_WINDOWS = 16384  # ICV_COPY_STATES_MAX_WINDOWS of include/infercnv_hip.h
MIN_STATES, MAX_STATES = 2, 8
DEFAULT_STEPS = (-2, -1, 0, 1, 2, 3)
VARIANTS = so.VARIANTS


# ---- rule 1 --------------------------------------------------------------------------------------------------------------
def check_levels(levels):
    """(list of K floats, z) of rule 1."""
    mu = [float(v) for v in levels]
    if not MIN_STATES <= len(mu) <= MAX_STATES:
        raise ValueError(f"cnv_copy_states: {len(mu)} states")
    if not all(math.isfinite(v) for v in mu):
        raise ValueError("cnv_copy_states: a level is not finite")
    for a, b in zip(mu[:-1], mu[1:]):
        if not b > a:
            raise ValueError("cnv_copy_states: the levels do not ascend strictly")
    zeros = [k for k, v in enumerate(mu) if v == 0.0]
    if len(zeros) != 1:
        raise ValueError("cnv_copy_states: not exactly one level is 0.0")
    mu[zeros[0]] = 0.0
    return mu, zeros[0]


def scalars(sigma, switch_prob, k):
    """(h, stay, sw) of rule 1 for k states."""
    return 1.0 / (2.0 * sigma * sigma), math.log(1.0 - switch_prob), math.log(switch_prob / (k - 1))


def end_order(k, z):
    """rule 4: z, z - 1, z + 1, z - 2, z + 2, ... inside [0, k)."""
    out = [z]
    for step in range(1, k):
        for s in (z - step, z + step):
            if 0 <= s < k:
                out.append(s)
    return out


def check_emissions(x, mu, sigma):
    """rule 6 on a canonical CSR matrix."""
    m = max((abs(v) for v in x.data.tolist()), default=0.0)
    h = 1.0 / (2.0 * sigma * sigma)
    t = m + max(abs(mu[0]), abs(mu[-1]))
    if not math.isfinite((t * t) * h):
        raise ValueError(f"cnv_copy_states: sigma={sigma!r} and levels={mu!r} overflow the emission of the value of "
                         f"magnitude {m!r}")


def largest_value_that_does_not_overflow(mu, sigma):
    """The largest float64 m that passes rule 6, by bisection on the rule itself."""
    h = 1.0 / (2.0 * sigma * sigma)
    top = max(abs(mu[0]), abs(mu[-1]))

    def ok(m):
        t = m + top
        return math.isfinite((t * t) * h)

    lo, hi = 1.0, 1e160
    assert ok(lo) and not ok(hi)
    while math.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2.0
        lo, hi = (mid, hi) if ok(mid) else (lo, mid)
    return lo


# ---- rules 2-4 -----------------------------------------------------------------------------------------------------------
def emissions(x, mu, h):
    """rule 2: [e_0 .. e_{K-1}] of one value."""
    out = []
    for m in mu:
        t = x - m
        out.append(-(t * t) * h)
    return out


def _emissions_emul(x, mu, h):
    """not rule 2: -(t (t h))."""
    out = []
    for m in mu:
        t = x - m
        out.append(-(t * (t * h)))
    return out


def _fma_add(best, x, m, h):
    """not rule 3: best + e with the product -(t t) h left unrounded (one fused multiply-add), exactly."""
    t = x - m
    return float(fractions.Fraction(best) - fractions.Fraction(t * t) * fractions.Fraction(h))


def viterbi_chain(xs, mu, z, h, stay, sw, variant=None):
    """rules 3-4 on the values of one chromosome: the list of states in [0, K).

    ``variant`` names a deviation that the tests show to be visible (never the contract), those of
    ``_states_oracle.viterbi_chain``: ``"assoc"`` adds ``d(r) + (T + e)``, ``"emul"`` forms ``-(t (t h))``, ``"fma"``
    fuses the product ``-(t t) h`` into the add."""
    assert variant is None or variant in VARIANTS
    emit = _emissions_emul if variant == "emul" else emissions
    k = len(mu)
    d = emit(xs[0], mu, h)
    back = []
    for x in xs[1:]:
        e = emit(x, mu, h)
        nd, arg = [], []
        for s in range(k):
            if variant == "assoc":
                best, who = d[s] + (stay + e[s]), s
                for r in range(k):
                    if r == s:
                        continue
                    cand = d[r] + (sw + e[s])
                    if cand > best:
                        best, who = cand, r
                nd.append(best)
                arg.append(who)
                continue
            best, who = d[s] + stay, s  # r = s first
            for r in range(k):  # then the others, the lower r first; only a strictly larger value replaces
                if r == s:
                    continue
                cand = d[r] + sw
                if cand > best:
                    best, who = cand, r
            nd.append(_fma_add(best, x, mu[s], h) if variant == "fma" else best + e[s])
            arg.append(who)
        d = nd
        back.append(arg)
    order = end_order(k, z)
    s = order[0]
    for c in order[1:]:
        if d[c] > d[s]:
            s = c
    path = [s]
    for arg in reversed(back):
        s = arg[s]
        path.append(s)
    path.reverse()
    return path


TWO_BEST_BUGS = ("no_demotion", "no_second", "first_for_all")


def viterbi_chain_two_best(xs, mu, z, h, stay, sw, bug=None):
    """rules 3-4 with rule 3 in the kernel's O(K) form (csrc/icv_copy_states.hpp): every state shares the candidates
    ``w_r = d(r) + sw``; ``a1`` / ``m1`` are the first r with the largest w_r and that value, ``a2`` / ``m2`` the same among
    the r != a1, both kept in one pass over ascending r in which only a strictly larger value replaces.  State s compares
    ``d(s) + stay`` with ``m1``, state a1 with ``m2``; a window's back-pointers are the set of states that stayed, a1 and
    a2.  Without ``bug`` the list of states is that of ``viterbi_chain``.

    ``bug`` plants one mistake in the bookkeeping of the second best (never the contract): ``"no_demotion"`` leaves
    m2 / a2 as they are when a new best is found, ``"no_second"`` never lets a later r become the second best,
    ``"first_for_all"`` compares state a1 with m1 like every other state (the backtrack still takes a2 for it).  None of them can show while
    ``stay >= sw``, that is ``switch_prob <= (K - 1) / K``: ``m2 <= m1 = d(a1) + sw <= d(a1) + stay``, so state a1 stays
    whatever m2 and a2 hold."""
    assert bug is None or bug in TWO_BEST_BUGS
    k = len(mu)
    d = emissions(xs[0], mu, h)
    back = []
    for x in xs[1:]:
        e = emissions(x, mu, h)
        m1, m2, a1, a2 = d[0] + sw, d[1] + sw, 0, 1
        if m2 > m1:
            m1, m2, a1, a2 = m2, m1, 1, 0
        for r in range(2, k):
            w = d[r] + sw
            if w > m1:
                if bug != "no_demotion":
                    m2, a2 = m1, a1
                m1, a1 = w, r
            elif w > m2 and bug != "no_second":
                m2, a2 = w, r
        nd, stayed = [], []
        for s in range(k):
            keep = d[s] + stay
            other = m2 if a1 == s and bug != "first_for_all" else m1
            left = other > keep
            nd.append((other if left else keep) + e[s])
            stayed.append(not left)
        d = nd
        back.append((stayed, a1, a2))
    order = end_order(k, z)
    s = order[0]
    for c in order[1:]:
        if d[c] > d[s]:
            s = c
    path = [s]
    for stayed, a1, a2 in reversed(back):
        if not stayed[s]:
            s = a2 if s == a1 else a1
        path.append(s)
    path.reverse()
    return path


def path_score(xs, path, mu, h, stay, sw):
    """The log-score of one path, summed in the order of rule 3: ((previous + T) + e)."""
    sc = emissions(xs[0], mu, h)[path[0]]
    for t in range(1, len(xs)):
        sc = (sc + (stay if path[t - 1] == path[t] else sw)) + emissions(xs[t], mu, h)[path[t]]
    return sc


# ---- the whole function ----------------------------------------------------------------------------------------------------
def cnv_copy_states(x, chr_pos, levels=None, amplitude=None, sigma=None, switch_prob=1e-3, bounds=None):
    """(states int8 n x W, sign int8 n x W, fraction float64 n, params dict) of rules 1-6."""
    if levels is not None and amplitude is not None:
        raise ValueError("cnv_copy_states: levels and amplitude are both given")
    x = so.canonical(x)
    n, w = x.shape
    if sigma is None:
        sigma = so.default_sigma(x)
    sigma = float(sigma)
    out = np.zeros((n, w), dtype=np.int8)
    if levels is None:
        if amplitude is None:
            amplitude = 2.0 * sigma
        mu, z = [float(k) * float(amplitude) for k in DEFAULT_STEPS], DEFAULT_STEPS.index(0)
        if sigma != 0.0:
            mu, z = check_levels(mu)
    else:
        mu, z = check_levels(levels)
    params = {"levels": list(mu), "neutral": z, "sigma": sigma, "switch_prob": float(switch_prob)}
    if sigma == 0.0:
        return out, out.copy(), np.zeros(n, dtype=np.float64), params
    h, stay, sw = scalars(sigma, float(switch_prob), len(mu))
    check_emissions(x, mu, sigma)
    edges = [int(v) for v in bounds] if bounds is not None else so.bounds(chr_pos, w)
    data, indices, indptr = x.data.tolist(), x.indices.tolist(), x.indptr.tolist()
    for i in range(n):
        row = [0.0] * w
        for k in range(indptr[i], indptr[i + 1]):
            row[indices[k]] = data[k]
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 > s0:
                out[i, s0:s1] = np.asarray(viterbi_chain(row[s0:s1], mu, z, h, stay, sw), dtype=np.int64) - z
    count = (out != 0).sum(axis=1)
    return out, np.sign(out).astype(np.int8), count.astype(np.float64) / float(w), params


# ---- case builders ---------------------------------------------------------------------------------------------------------
PLANTED_LENGTHS = (60, 1, 40, 29)
PLANTED_ROWS = 24
PLANTED_STEP = 0.3
PLANTED_EVENTS = ((10, 22, 1), (30, 42, 2), (70, 80, -1), (105, 113, 3))  # [first, last) window and copies gained
PLANTED_KWARGS = {"levels": (-0.6, -0.3, 0.0, 0.3, 0.6, 0.9), "sigma": 0.1, "switch_prob": 1e-3}
PLANTED_MOST_WRONG = 40    # the six-state chain, of 3 120 calls
PLANTED_LEAST_WRONG = 480  # the three-state chain: the windows with |truth| > 1


def planted_levels(seed):
    """The planted multi-level matrix: 24 dense rows of N(0, 0.1) over chromosomes of (60, 1, 40, 29) windows plus
    0.3 x truth, truth the same in every row: +1 on [10, 22), +2 on [30, 42), -1 on [70, 80), +3 on [105, 113).
    dict(x=dense float64, chr_pos, truth=int8 n x W, kwargs)."""
    rng = np.random.default_rng(seed)
    w = sum(PLANTED_LENGTHS)
    x = rng.normal(0.0, 0.1, (PLANTED_ROWS, w))
    truth = np.zeros((PLANTED_ROWS, w), dtype=np.int8)
    for a, b, v in PLANTED_EVENTS:
        truth[:, a:b] = v
    x = x + PLANTED_STEP * truth
    return {"x": x, "chr_pos": so.chr_pos_of(PLANTED_LENGTHS), "truth": truth, "kwargs": dict(PLANTED_KWARGS)}


def every_k_levels(k, z):
    """levels (s - z) / 2 for s in [0, k): with sigma = 0.25 (h = 8) every emission of a multiple of 0.25 is exact."""
    return [(s - z) * 0.5 for s in range(k)]


EVERY_K_KWARGS = {"sigma": 0.25}
EVERY_K_SWITCH = (1e-3, 0.3)


def every_k(k, z, switch_prob):
    """About 40 rows over the chromosome lengths of ``_states_oracle.ties``, the values multiples of 0.25 from one step
    (0.5) below the lowest level to one step above the highest: two states emit the same half-way between them, and
    paths tie.  Rows of one repeated value, seeded draws over the whole range and over the three values round neutral;
    every third row is fully stored, explicit zeros stay stored, one row is all zeros with nothing stored.
    dict(x=canonical CSR, chr_pos, kwargs)."""
    import scipy.sparse as sp

    w = sum(so.TIES_LENGTHS)
    lo, hi = (0 - z) * 0.5 - 0.5, (k - 1 - z) * 0.5 + 0.5
    vals = np.arange(int(round((hi - lo) / 0.25)) + 1) * 0.25 + lo
    rng = np.random.default_rng(100 * k + 10 * z + (1 if switch_prob > 0.01 else 0))
    rows = [np.full(w, v) for v in vals[::2]][:12]
    rows += [vals[rng.integers(0, len(vals), size=w)] for _ in range(20)]
    rows += [np.repeat(vals[rng.integers(0, len(vals), size=(w + 2) // 3)], 3)[:w] for _ in range(6)]
    stored = [np.ones(w, dtype=bool) if i % 3 == 0 else (r != 0.0) | (rng.random(w) < 0.3) for i, r in enumerate(rows)]
    rows.append(np.zeros(w))
    stored.append(np.zeros(w, dtype=bool))
    data, indices, indptr = [], [], [0]
    for r, m in zip(rows, stored):
        m = m | (r != 0.0)
        cols = np.flatnonzero(m)
        data.extend(r[cols].tolist())
        indices.extend(cols.tolist())
        indptr.append(len(data))
    x = sp.csr_matrix((np.asarray(data, dtype=np.float64), np.asarray(indices, dtype=np.int32),
                       np.asarray(indptr, dtype=np.int64)), shape=(len(rows), w))
    return {"x": x, "chr_pos": so.chr_pos_of(so.TIES_LENGTHS),
            "kwargs": dict(EVERY_K_KWARGS, levels=every_k_levels(k, z), switch_prob=switch_prob)}


HIGH_SWITCH = 0.999  # above (K - 1) / K for every K <= 8: sw > stay, and the best other state can beat staying in a1


def high_switch_positions(k):
    """The neutral positions of the HIGH_SWITCH cases: the first, the middle and the last state."""
    return sorted({0, k // 2, k - 1})


def chains_of(c):
    """[(row, first window, the chromosome's values as a list)] of a case: every chain the kernel runs."""
    dense = c["x"].toarray()
    edges = so.bounds(c["chr_pos"], dense.shape[1])
    return [(i, s0, dense[i, s0:s1].tolist()) for i in range(dense.shape[0]) for s0, s1 in zip(edges[:-1], edges[1:])]


def contract_chains(c):
    """[(the chromosome's values, the states ``viterbi_chain`` gives them)] over ``chains_of(c)``."""
    kw = c["kwargs"]
    mu, z = check_levels(kw["levels"])
    h, stay, sw = scalars(kw["sigma"], kw["switch_prob"], len(mu))
    return [(xs, viterbi_chain(xs, mu, z, h, stay, sw)) for _, _, xs in chains_of(c)]


def two_best_differences(c, bug=None, contract=None):
    """The number of the case's chains on which ``viterbi_chain_two_best(bug=)`` does not give the states of
    ``viterbi_chain``; ``contract`` takes a ``contract_chains(c)`` computed before."""
    kw = c["kwargs"]
    mu, z = check_levels(kw["levels"])
    h, stay, sw = scalars(kw["sigma"], kw["switch_prob"], len(mu))
    contract = contract_chains(c) if contract is None else contract
    return sum(viterbi_chain_two_best(xs, mu, z, h, stay, sw, bug) != want for xs, want in contract)


END_RULE_STATES = 8


def end_rule(z):
    """Rule 4 by hand, K = 8 with the neutral state at z: one row of seven one-window chromosomes, window s holding the
    value half-way between the levels s and s + 1 of ``every_k_levels(8, z)``.  With sigma = 0.25 (h = 8) the two
    emissions are exactly -0.5 and every other one is lower, so rule 4's order alone decides: the state nearer to z is
    tried first and a tie does not replace it, and z wins against both its neighbours.  ``want`` is written down from
    that, without the oracle.  dict(x, chr_pos, kwargs, want=int8 1 x 7)."""
    k = END_RULE_STATES
    mu = every_k_levels(k, z)
    x = np.array([[mu[s] + 0.25 for s in range(k - 1)]])
    want = np.array([[(s + 1 if s + 1 <= z else s) - z for s in range(k - 1)]], dtype=np.int8)
    return {"x": so.canonical(x), "chr_pos": so.chr_pos_of([1] * (k - 1)),
            "kwargs": dict(EVERY_K_KWARGS, levels=mu, switch_prob=1e-3), "want": want}


UNEQUAL_KWARGS = {"levels": (-0.7, -0.15, 0.0, 0.4, 0.45, 1.3, 2.0), "sigma": 0.17, "switch_prob": 0.01}
UNEQUAL_LENGTHS = (37, 1, 64, 29)  # W = 131: no multiple of 4 or 64


def unequal_levels():
    """Seven levels that are no multiples of one step, two of them 0.05 apart, under a sigma with nothing dyadic: every
    operation of rules 2-3 rounds, and no symmetry of the lattice hides a state taken for its neighbour.  14 rows of
    N(0, 0.17) plus one level per stretch of 4 .. 12 windows, drawn from all seven; a third of the values is not stored.
    dict(x, chr_pos, kwargs)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(77)
    w = sum(UNEQUAL_LENGTHS)
    mu = np.asarray(UNEQUAL_KWARGS["levels"])
    dense = rng.normal(0.0, UNEQUAL_KWARGS["sigma"], size=(14, w))
    for i in range(dense.shape[0]):
        t = 0
        while t < w:
            n = int(rng.integers(4, 13))
            dense[i, t:t + n] += mu[rng.integers(0, len(mu))]
            t += n
    dense[rng.random(dense.shape) < 1.0 / 3.0] = 0.0
    return {"x": sp.csr_matrix(dense), "chr_pos": so.chr_pos_of(UNEQUAL_LENGTHS), "kwargs": dict(UNEQUAL_KWARGS)}


ROUNDING_LENGTHS = (2, 3, 6)
ROUNDING_CHAINS = 400  # per length
ROUNDING_ROWS = 4
ROUNDING_SEED = 1
ROUNDING_A, ROUNDING_SIGMA = 0.23, 0.1  # nothing dyadic: every operation rounds
ROUNDING_KWARGS = {"levels": tuple(float(k) * ROUNDING_A for k in DEFAULT_STEPS), "sigma": ROUNDING_SIGMA,
                   "switch_prob": 1e-3}


def rounding_ties(seed=ROUNDING_SEED):
    """The K = 6 rounding case: chains in which the last bit of the sums decides between two gain levels.  A chain of L
    windows has L - 1 values ``1.5 a + N(0, sigma / 2)`` and a last value of ``L 1.5 a`` minus their sum: in exact
    arithmetic the all-(+1) and the all-(+2) path score the same.  400 chains of each L in (2, 3, 6), 100 of each per
    row (300 chromosomes a row: the lanes take several each); the odd rows are mirrored (-x).
    dict(x, chr_pos, kwargs, chains={L: [(row, first window)]})."""
    rng = random.Random(seed)
    a, sigma = ROUNDING_A, ROUNDING_SIGMA
    per_row = ROUNDING_CHAINS // ROUNDING_ROWS
    lengths = [L for L in ROUNDING_LENGTHS for _ in range(per_row)]
    w = sum(lengths)
    dense = np.zeros((ROUNDING_ROWS, w))
    chains = {L: [] for L in ROUNDING_LENGTHS}
    for i in range(ROUNDING_ROWS):
        t = 0
        for L in lengths:
            xs = [1.5 * a + rng.gauss(0.0, sigma / 2) for _ in range(L - 1)]
            xs.append(L * 1.5 * a - sum(xs))
            dense[i, t:t + L] = xs
            chains[L].append((i, t))
            t += L
    dense[1::2] *= -1.0
    return {"x": so.canonical(dense), "chr_pos": so.chr_pos_of(lengths), "kwargs": dict(ROUNDING_KWARGS),
            "chains": chains}


def rounding_differences(c, variant):
    """{L: the number of the case's chains of L windows whose calls under ``variant`` are not the contract's}."""
    dense = c["x"].toarray()
    kw = c["kwargs"]
    mu, z = check_levels(kw["levels"])
    h, stay, sw = scalars(kw["sigma"], kw["switch_prob"], len(mu))
    out = {}
    for L, where in c["chains"].items():
        n = 0
        for i, t in where:
            xs = dense[i, t:t + L].tolist()
            n += viterbi_chain(xs, mu, z, h, stay, sw) != viterbi_chain(xs, mu, z, h, stay, sw, variant)
        out[L] = n
    return out


SPLIT_LEVELS = tuple(float(k) * so.TIES_A for k in DEFAULT_STEPS)


def output_split(w):
    """``_states_oracle.output_split(w)`` with every value doubled or tripled here and there: 9 rows of w windows from
    {0, +-a, +-2a, +3a}, the first and the last window never 0, under the six levels k a and switch_prob = 0.3: most
    calls are not 0 and several are beyond +-1, so the two planes differ, and rows follow each other w bytes apart.
    dict(x, chr_pos, kwargs)."""
    base = so.output_split(w)
    dense = base["x"].toarray()
    rng = np.random.default_rng(2000 + w)
    scale = rng.choice([1.0, 2.0, 3.0], size=dense.shape, p=[0.4, 0.4, 0.2])
    dense = np.where(dense > 0, dense * scale, dense * np.minimum(scale, 2.0))
    return {"x": so.canonical(dense), "chr_pos": base["chr_pos"],
            "kwargs": {"levels": SPLIT_LEVELS, "sigma": 0.25, "switch_prob": 0.3}}


def shapes():
    """Chromosome layouts at which the kernel takes another path, the rows of ``_states_oracle.planted`` called with
    the six default levels: {name: case}."""
    rng = np.random.default_rng(11)
    many65 = rng.integers(1, 7, size=65).tolist()
    many130 = rng.integers(1, 7, size=130).tolist()
    return {
        "single_chromosome": so.planted(5, [50], 1),
        "one_window": so.planted(3, [1], 2, keep=0.5),
        "one_window_chromosome_between_long": so.planted(9, [30, 1, 30], 3),
        "chromosomes_65": so.planted(7, many65, 4),
        "chromosomes_130": so.planted(6, many130, 5),
        "max_windows": so.planted(2, [9000, 5000, MAX_WINDOWS - 14000], 6),
    }


SHAPE_NAMES = ("single_chromosome", "one_window", "one_window_chromosome_between_long", "chromosomes_65",
               "chromosomes_130", "max_windows")
SHAPE_KWARGS = {"amplitude": 0.3, "sigma": 0.1}  # planted() shifts by 6 s = 0.6: two steps of 0.3


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its expected output, computed once:
    dict(x, chr_pos, kwargs, states, sign, fraction, params)."""
    if name == "rounding_ties":
        c = rounding_ties()
    elif name.startswith("output_split_"):
        c = output_split(int(name[len("output_split_"):]))
    elif name.startswith("planted_levels_"):
        c = planted_levels(int(name[len("planted_levels_"):]))
    elif name.startswith("every_k_"):
        k, z, p = name[len("every_k_"):].split("_")
        c = every_k(int(k), int(z), float(p))
    elif name.startswith("end_rule_"):
        c = end_rule(int(name[len("end_rule_"):]))
    elif name == "unequal_levels":
        c = unequal_levels()
    else:
        c = shapes()[name]
        c["kwargs"] = dict(SHAPE_KWARGS)
    c["states"], c["sign"], c["fraction"], c["params"] = cnv_copy_states(c["x"], c["chr_pos"], **c["kwargs"])
    for v in (c["states"], c["sign"], c["fraction"]):
        v.setflags(write=False)
    return c

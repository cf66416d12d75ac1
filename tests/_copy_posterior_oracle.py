"""Numpy oracle of tl.cnv_copy_posteriors and tl.cnv_copy_states_filter, and the builders of their test
cases.

Posteriors: the K-state form of ``_posterior_oracle``.  All arithmetic is IEEE float64 without fused multiply-add, one
numpy operation per written operation (the cells are the vector axis, the windows and the states explicit loops):

1. ``h = 1.0 / (2.0 sigma sigma)``, ``ps = 1.0 - p``, ``pw = p / (K - 1)``; ``A(r, s) = ps`` for r = s, ``pw`` otherwise.
   The levels follow rule 1 of ``_copy_states_oracle``: 2 <= K <= 8, strictly ascending, exactly one 0.0 at index z.
2. ``t = x - mu_s; e_s = -(t t) h``; ``m = e_0``, then for s = 1 .. K-1 ``if e_s > m: m = e_s``;
   ``b(s) = exp_(e_s - m)`` with the written exponential of ``_tsne_oracle``.
3. Forward: ``u_0(s) = b_0(s)``; for t >= 1 ``pred(s) = (..((al(0) A(0,s)) + (al(1) A(1,s))) + ..) + (al(K-1) A(K-1,s))``
   over ``al_{t-1}``, r ascending, and ``u_t(s) = pred(s) b_t(s)``; ``c_t = (..(u(0) + u(1)) + ..) + u(K-1)``,
   ``al_t(s) = u_t(s) / c_t`` (at t = 0 the same c and division apply to u_0).
4. Backward: ``be_{T-1}(s) = 1.0``; ``g(s) = b_{t+1}(s) be_{t+1}(s)``,
   ``v(r) = (..((A(r,0) g(0)) + (A(r,1) g(1))) + ..)``, s ascending, ``be_t(r) = v(r) / c_{t+1}``.
5. ``w(s) = al_t(s) be_t(s)``, ``z = (..(w(0) + w(1)) + ..)``, ``gamma_t(s) = w(s) / z``.
6. Chains never cross a chromosome boundary; an entry that is not stored is 0.0; a window that no chromosome covers has
   gamma = 1.0 for state z and 0.0 elsewhere.
7. Overflow: rule 6 of ``_copy_states_oracle`` under the amplitude ``max(|levels[0]|, |levels[-1]|)``.

The K^2 sums of rules 3 and 4 are the contract.  ``DEVIATIONS`` names three other ways to form them, which are never the
contract; the tests show each of them to be visible on the GPU parity set.

Filter.  ``q_t = int64(rint(P[i,t] 2^40))``; a run ``[s, e)`` (a maximal stretch of ONE level other than 0 inside one
chromosome: ``+1 +1 +2 +2`` is two runs) has ``S = sum q_t`` (an integer) and ``mean = float(S) / (float(e - s) 2^40)``;
it is reset to 0 iff ``mean > max_p_normal``.  Levels lie in [-7, 7].
"""
import fractions
import functools

import numpy as np

import _copy_states_oracle as co
import _posterior_oracle as po
import _states_oracle as so
from _tsne_oracle import exp_

LDS_BYTES = 163840  # ICV_COPY_POSTERIOR_LDS_BYTES of include/infercnv_hip.h
MIN_STATES, MAX_STATES = co.MIN_STATES, co.MAX_STATES
MAX_LEVEL = 7
TWO40 = po.TWO40
DEVIATIONS = ("ok_form", "descending", "fma")


def max_windows(k):
    """ICV_COPY_POSTERIOR_MAX_WINDOWS(k) of include/infercnv_hip.h."""
    return LDS_BYTES // (8 * (k + 1))


def plane_names(k, z):
    return [f"loss{z - s}" if s < z else "neutral" if s == z else f"gain{s - z}" for s in range(k)]


# ---- posteriors ------------------------------------------------------------------------------------------------------------
def scalars(sigma, switch_prob, k):
    """(h, ps, pw) of rule 1 for k states."""
    return 1.0 / (2.0 * sigma * sigma), 1.0 - switch_prob, switch_prob / (k - 1)


def emissions(x, mu, h):
    """rule 2: [b(0) .. b(K-1)] of a float64 vector of values."""
    e = []
    for m in mu:
        t = x - m
        e.append(-(t * t) * h)
    top = e[0]
    for v in e[1:]:
        top = np.where(v > top, v, top)
    return [exp_(v - top) for v in e]


def _fma(a, b, c):
    """a b + c with one rounding, exactly (not a rule: the "fma" deviation)."""
    one = np.frompyfunc(lambda x, y, w: float(fractions.Fraction(x) * fractions.Fraction(y) + fractions.Fraction(w)), 3, 1)
    return one(a, b, c).astype(np.float64)


def _mix(y, coef, deviation=None):
    """(..((y(0) coef(0)) + (y(1) coef(1))) + ..): the sums of rules 3 and 4 with the row or column ``coef`` of A.

    ``deviation`` (never the contract): ``"descending"`` runs the sum from K - 1 down, ``"fma"`` fuses each product into
    the add that takes it."""
    k = len(y)
    order = range(k - 1, -1, -1) if deviation == "descending" else range(k)
    acc = None
    for r in order:
        if acc is None:
            acc = y[r] * coef[r]
        elif deviation == "fma":
            acc = _fma(y[r], np.full_like(y[r], coef[r]), acc)
        else:
            acc = acc + (y[r] * coef[r])
    return acc


def _sum(v):
    acc = v[0]
    for u in v[1:]:
        acc = acc + u
    return acc


def _pred(al, ps, pw, deviation):
    k = len(al)
    if deviation == "ok_form":  # not rule 3: the O(K) rewrite al(s) ps + (S - al(s)) pw
        total = _sum(al)
        return [(al[s] * ps) + ((total - al[s]) * pw) for s in range(k)]
    return [_mix(al, [ps if r == s else pw for r in range(k)], deviation) for s in range(k)]


def chain(xs, mu, h, ps, pw, deviation=None):
    """rules 2-5 on one chromosome of many cells: xs float64 (n, T) -> gamma float64 (K, n, T).  ``deviation`` names one
    of DEVIATIONS, applied to pred of rule 3 (forward and, for c, backward) and, but for ``"ok_form"``, to v of rule 4."""
    assert deviation is None or deviation in DEVIATIONS
    xs = np.asarray(xs, dtype=np.float64)
    n, T = xs.shape
    k = len(mu)
    b = [emissions(xs[:, t], mu, h) for t in range(T)]
    al, cs = [], []
    for t in range(T):
        if t == 0:
            u = list(b[0])
        else:
            pred = _pred(al[-1], ps, pw, deviation)
            u = [pred[s] * b[t][s] for s in range(k)]
        c = _sum(u)
        al.append([u[s] / c for s in range(k)])
        cs.append(c)
    gamma = np.empty((k, n, T), dtype=np.float64)
    be = [np.ones(n) for _ in range(k)]
    back = None if deviation == "ok_form" else deviation
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            g = [b[t + 1][s] * be[s] for s in range(k)]
            # (A(r,s) g(s): the product commutes, the order of the sum is that of _mix)
            v = [_mix(g, [ps if r == s else pw for s in range(k)], back) for r in range(k)]
            be = [v[r] / cs[t + 1] for r in range(k)]
        w = [al[t][s] * be[s] for s in range(k)]
        z = _sum(w)
        for s in range(k):
            gamma[s, :, t] = w[s] / z
    return gamma


def resolve_levels(x, levels, amplitude, sigma):
    """(mu, z, sigma) as ``_copy_states_oracle.cnv_copy_states`` resolves them; x canonical."""
    if levels is not None and amplitude is not None:
        raise ValueError("cnv_copy_posteriors: levels and amplitude are both given")
    if sigma is None:
        sigma = so.default_sigma(x)
    sigma = float(sigma)
    if levels is None:
        if amplitude is None:
            amplitude = 2.0 * sigma
        mu, z = [float(k) * float(amplitude) for k in co.DEFAULT_STEPS], co.DEFAULT_STEPS.index(0)
        if sigma != 0.0:
            mu, z = co.check_levels(mu)
    else:
        mu, z = co.check_levels(levels)
    return mu, z, sigma


def cnv_copy_posteriors(x, chr_pos, levels=None, amplitude=None, sigma=None, switch_prob=None, bounds=None,
                        deviation=None):
    """(planes float64 K x n x W in state order, params dict); planes[params["neutral"]] is P(neutral)."""
    x = so.canonical(x)
    n, w = x.shape
    mu, z, sigma = resolve_levels(x, levels, amplitude, sigma)
    if switch_prob is None:
        switch_prob = 1e-3
    k = len(mu)
    params = {"levels": list(mu), "neutral": z, "sigma": sigma, "switch_prob": float(switch_prob)}
    out = np.zeros((k, n, w), dtype=np.float64)
    out[z] = 1.0
    if sigma == 0.0:
        return out, params
    co.check_emissions(x, mu, sigma)
    h, ps, pw = scalars(sigma, float(switch_prob), k)
    dense = x.toarray()
    edges = [int(v) for v in bounds] if bounds is not None else so.bounds(chr_pos, w)
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 > s0:
                out[:, :, s0:s1] = chain(dense[:, s0:s1], mu, h, ps, pw, deviation)
    return out, params


def log_space_posteriors(xs, mu, sigma, switch_prob):
    """An independent forward-backward in log space (``np.logaddexp``, no scaling, no written exponential) on one
    chromosome of many cells: xs (n, T) -> gamma (K, n, T)."""
    xs = np.asarray(xs, dtype=np.float64)
    n, T = xs.shape
    k = len(mu)
    le = np.stack([-((xs - m) ** 2) / (2.0 * sigma * sigma) for m in mu])  # (K, n, T)
    la = np.full((k, k), np.log(switch_prob / (k - 1)))
    la[np.arange(k), np.arange(k)] = np.log1p(-switch_prob)
    fwd = np.empty((k, n, T))
    fwd[:, :, 0] = le[:, :, 0]
    for t in range(1, T):
        for s in range(k):
            fwd[s, :, t] = np.logaddexp.reduce([fwd[r, :, t - 1] + la[r, s] for r in range(k)], axis=0) + le[s, :, t]
    bwd = np.zeros((k, n, T))
    for t in range(T - 2, -1, -1):
        for r in range(k):
            bwd[r, :, t] = np.logaddexp.reduce([la[r, s] + le[s, :, t + 1] + bwd[s, :, t + 1] for s in range(k)], axis=0)
    lg = fwd + bwd
    return np.exp(lg - np.logaddexp.reduce(lg, axis=0))


# ---- filter ----------------------------------------------------------------------------------------------------------------
def copy_states_filter(states, p_neutral, chr_pos, max_p_normal=0.5):
    """(filtered int8 n x W, sign int8 n x W, fraction float64 n, removed int32 n, means): ``means`` lists
    (row, start, end, mean) of every run."""
    states = np.asarray(states)
    p = np.asarray(p_neutral, dtype=np.float64)
    if ((states < -MAX_LEVEL) | (states > MAX_LEVEL)).any():
        raise ValueError("a level outside [-7, 7]")
    if not ((p >= 0.0) & (p <= 1.0)).all():
        raise ValueError("a posterior that is not a number in [0, 1]")
    n, w = states.shape
    q = np.rint(p * TWO40).astype(np.int64)
    edges = so.bounds(chr_pos, w)
    out = states.astype(np.int8).copy()
    removed = np.zeros(n, dtype=np.int32)
    means = []
    for i in range(n):
        for s, e in po.runs(states[i], edges):  # (a run ends where the level changes)
            total = sum(q[i, s:e].tolist())  # a Python integer
            mean = float(total) / (float(e - s) * TWO40)
            means.append((i, s, e, mean))
            if mean > max_p_normal:
                out[i, s:e] = 0
                removed[i] += 1
    return out, np.sign(out).astype(np.int8), (out != 0).sum(axis=1).astype(np.float64) / float(w), removed, means


def crafted_filter_cases():
    """{name: dict(states int8, p float64, chr_pos, max_p_normal, want int8)}: the verdicts on levels that a run defined
    by the sign, a wrong comparison or a run across a chromosome boundary would get wrong."""
    half = np.full((1, 8), 0.5)
    twos = np.array([[0, 2, 2, 2, 2, 2, 0, 0]], dtype=np.int8)
    return {
        "two_levels_of_one_sign_are_two_runs": dict(
            states=np.array([[1, 1, 2, 2, 0]], dtype=np.int8), p=np.array([[0.9, 0.9, 0.1, 0.1, 0.3]]),
            chr_pos={"a": 0}, max_p_normal=0.5, want=np.array([[0, 0, 2, 2, 0]], dtype=np.int8)),
        "two_levels_whose_joint_mean_would_stay": dict(  # one run of four would have the mean 0.4 and stay whole
            states=np.array([[-2, -2, -1, -1, 0]], dtype=np.int8), p=np.array([[0.7, 0.7, 0.1, 0.1, 0.3]]),
            chr_pos={"a": 0}, max_p_normal=0.5, want=np.array([[0, 0, -1, -1, 0]], dtype=np.int8)),
        "mean_equal_to_the_threshold_stays": dict(states=twos, p=half, chr_pos={"a": 0}, max_p_normal=0.5, want=twos),
        "mean_2^-30_above_goes": dict(states=twos, p=half + 2.0 ** -30, chr_pos={"a": 0}, max_p_normal=0.5,
                                     want=np.zeros_like(twos)),
        "chromosome_boundary_cuts_a_run_of_one_level": dict(
            states=np.array([[3, 3, 3, 3, 3, 3]], dtype=np.int8), p=np.array([[0.9, 0.9, 0.9, 0.1, 0.1, 0.1]]),
            chr_pos={"a": 0, "b": 3}, max_p_normal=0.5, want=np.array([[0, 0, 0, 3, 3, 3]], dtype=np.int8)),
        "the_widest_levels": dict(
            states=np.array([[-7, -7, 7, 7, 0]], dtype=np.int8), p=np.array([[0.1, 0.1, 0.9, 0.9, 0.3]]),
            chr_pos={"a": 0}, max_p_normal=0.5, want=np.array([[-7, -7, 0, 0, 0]], dtype=np.int8)),
    }


def doubled(case):
    """A case of ``_posterior_oracle`` (calls in -1 / 0 / +1) with every call multiplied by 2: the same runs."""
    return dict(case, states=(np.asarray(case["states"]).astype(np.int16) * 2).astype(np.int8))


def alternating(case):
    """A sweep case of ``_posterior_oracle`` whose neighbour runs (every called window outside the rows' main runs)
    alternate between the levels 1 and 2 of their sign window by window: every such window is a run of its own."""
    states = np.asarray(case["states"]).copy()
    for i, (s, e) in enumerate(case["main"]):
        outside = np.ones(states.shape[1], dtype=bool)
        outside[s:e] = False
        level = 1 + (np.arange(states.shape[1]) % 2)
        states[i] = np.where(outside, states[i] * level, states[i]).astype(np.int8)
    return dict(case, states=states)


# ---- cases -----------------------------------------------------------------------------------------------------------------
SHAPE_NAMES = tuple(name for name in co.SHAPE_NAMES if name != "max_windows")
SHAPE_KWARGS = dict(co.SHAPE_KWARGS)
# The chain cnv_copy_states -> cnv_copy_posteriors -> cnv_copy_states_filter -> cnv_segments on the planted multi-level
# case of DESIGN.md 4.22, seed 2, at max_p_normal = 0.2.  The six-state chain leaves 16 wrong calls of 3 120.  The filter
# removes exactly two runs, both of one window and both false calls (means about 0.355 and 0.213), and keeps every run
# whose call is right (the largest such mean is about 0.078): the wrong calls go from 16 to 14.
# test_copy_posterior_oracle.py checks that.
CHAIN_SEED, CHAIN_MAX_P_NORMAL = 2, 0.2
CHAIN_REMOVED_MEANS = (0.355, 0.213)
CHAIN_LARGEST_RIGHT_MEAN = 0.078
CHAIN_WRONG_BEFORE, CHAIN_WRONG_AFTER = 16, 14


def cap_case(k):
    """2 rows of max_windows(k) windows in one chromosome under k levels with the neutral one in the middle."""
    w = max_windows(k)
    c = so.planted(2, [w], 60 + k)
    c["kwargs"] = {"levels": [(s - k // 2) * 0.3 for s in range(k)], "sigma": 0.1, "switch_prob": 1e-3}
    return c


CUTOFF5_KWARGS = {"levels": (-1.0, -0.5, 0.0, 0.5, 1.0), "sigma": 0.25, "switch_prob": 1e-3}  # h = 8: exact emissions
CUTOFF5_VALUES = (44.6875, 44.75, 44.8125)  # e_neutral - e_top = -707, -708 (ts_exp's last non-zero argument) and -709
CUTOFF5_GAPS = (-707.0, -708.0, -709.0)


def exp_cutoff5():
    """``_posterior_oracle.exp_cutoff`` for five levels, the neutral one in the middle: rule 2's ``m`` is the largest of
    five emissions.  At x = +v the top state has b = 1.0, the state below it b = exp_(1 - 8 v) (about 1e-153), the neutral
    state b = exp_ of CUTOFF5_GAPS and the two loss states lie far beyond the cutoff (exactly 0.0): a window holds
    several exact zeros and one smallest b that is not 0.  The layout is that of ``exp_cutoff``: rows 0-5 hold one value
    (+ and - of each) at the CUTOFF_PROBES windows among windows on that sign's outermost level, rows 6-11 the same among
    windows that are not stored, then extremes of both signs side by side, and noise.  Every value is a float32 number.
    dict(x, chr_pos, kwargs, probes=[(row, window, |value|)])."""
    import scipy.sparse as sp

    mu, z = co.check_levels(CUTOFF5_KWARGS["levels"])
    h = scalars(CUTOFF5_KWARGS["sigma"], CUTOFF5_KWARGS["switch_prob"], len(mu))[0]
    assert h == 8.0 and z == 2
    for v, gap in zip(CUTOFF5_VALUES, CUTOFF5_GAPS):
        for sign in (1.0, -1.0):
            e = co.emissions(sign * v, mu, h)
            top = e[-1] if sign > 0 else e[0]
            assert top == max(e) and e[z] - top == gap and all(fractions.Fraction(-w / h).denominator <= 256 for w in e)
    top = mu[-1]
    w = sum(po.CUTOFF_LENGTHS)
    lo, mid, hi = CUTOFF5_VALUES
    rows, probes = [], []
    for background in (top, 0.0):
        for v in CUTOFF5_VALUES:
            for sign in (1.0, -1.0):
                row = np.full(w, sign * background)
                row[list(po.CUTOFF_PROBES)] = sign * v
                if background:
                    probes.extend((len(rows), t, v) for t in po.CUTOFF_PROBES)
                rows.append(row)
    row = np.zeros(w)
    row[0:6] = [hi, -hi, mid, -mid, lo, -lo]  # the chain meets states it gave probability 0
    row[10:14] = [mid, mid, hi, hi]
    row[18:23] = [-lo, 0.5, -mid, -0.5, -hi]
    rows.append(row)
    rng = np.random.default_rng(43)
    for v in CUTOFF5_VALUES:
        row = rng.normal(0.0, 0.5, size=w).astype(np.float32).astype(np.float64)
        row[rng.random(w) < 0.4] = 0.0
        row[rng.integers(0, w, size=3)] = [v, -v, v]
        rows.append(row)
    dense = np.vstack(rows)
    assert np.array_equal(dense, dense.astype(np.float32).astype(np.float64))
    return {"x": sp.csr_matrix(dense), "chr_pos": so.chr_pos_of(po.CUTOFF_LENGTHS), "kwargs": dict(CUTOFF5_KWARGS),
            "probes": probes}


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its expected output, computed once: dict(x, chr_pos, kwargs, planes, params)."""
    if name == "exp_cutoff5":
        c = exp_cutoff5()
    elif name == "unequal_levels":
        c = co.unequal_levels()
    elif name.startswith("every_k_"):
        k, z, p = name[len("every_k_"):].split("_")
        c = co.every_k(int(k), int(z), float(p))
    elif name.startswith("planted_levels_"):
        c = co.planted_levels(int(name[len("planted_levels_"):]))
    elif name.startswith("cap_"):
        c = cap_case(int(name[len("cap_"):]))
    else:
        c = co.shapes()[name]
        c["kwargs"] = dict(SHAPE_KWARGS)
    c["planes"], c["params"] = cnv_copy_posteriors(c["x"], c["chr_pos"], **c["kwargs"])
    c["planes"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def chain_case():
    """The oracle chain on the planted case: dict(x, chr_pos, truth, kwargs, states, planes, neutral, filtered, sign,
    fraction, removed, means)."""
    c = dict(case(f"planted_levels_{CHAIN_SEED}"))
    c["states"], _, _, params = co.cnv_copy_states(c["x"], c["chr_pos"], **c["kwargs"])
    assert params == c["params"]
    c["neutral"] = c["planes"][params["neutral"]]
    c["filtered"], c["sign"], c["fraction"], c["removed"], c["means"] = copy_states_filter(
        c["states"], c["neutral"], c["chr_pos"], CHAIN_MAX_P_NORMAL)
    for key in ("states", "filtered", "sign", "fraction", "removed"):
        c[key].setflags(write=False)
    return c

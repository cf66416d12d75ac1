"""Numpy oracle of tl.cnv_posteriors and tl.cnv_states_filter, and the builders of their test cases.

Posteriors.  All arithmetic is IEEE float64 without fused multiply-add, one numpy operation per written operation (the
cells are the vector axis, the windows an explicit loop):

1. ``h = 1.0 / (2.0 sigma sigma)``, ``ps = 1.0 - p``, ``pw = p / 2.0``; ``A(r, s) = ps`` for r = s, ``pw`` otherwise.
2. ``t = x - mu_s; e_s = -(t t) h`` for the means (-a, 0.0, +a); ``m = max(e_0, e_1, e_2)``;
   ``b(s) = exp_(e_s - m)`` with the written exponential of ``_tsne_oracle``.
3. Forward: ``u_0(s) = b_0(s)``; for t >= 1 ``pred(s) = ((al(0) A(0,s)) + (al(1) A(1,s))) + (al(2) A(2,s))`` over
   ``al_{t-1}`` and ``u_t(s) = pred(s) b_t(s)``; ``c_t = (u(0) + u(1)) + u(2)``, ``al_t(s) = u_t(s) / c_t``.
4. Backward: ``be_{T-1}(s) = 1.0``; ``g(s) = b_{t+1}(s) be_{t+1}(s)``,
   ``v(r) = ((A(r,0) g(0)) + (A(r,1) g(1))) + (A(r,2) g(2))``, ``be_t(r) = v(r) / c_{t+1}``.
5. ``w(s) = al_t(s) be_t(s)``, ``z = (w(0) + w(1)) + w(2)``, ``gamma_t(s) = w(s) / z``.
6. Chains never cross a chromosome boundary; an entry that is not stored is 0.0.
7. Overflow: rule 6 of ``_states_oracle`` (a ``(m + a)^2 h`` that is not finite is a ``ValueError``).

``bounds=`` takes the kernel's own ``chr_start`` array in place of ``chr_pos`` as in ``_states_oracle``: a chromosome with
``s1 <= s0`` is skipped, a window that no chromosome covers has the posterior (0, 1, 0).

Filter.  ``q_t = int64(rint(P[i,t] 2^40))``; a run ``[s, e)`` (a maximal stretch of -1 or of +1 inside one chromosome)
has ``S = sum q_t`` (an integer) and ``mean = float(S) / (float(e - s) 2^40)``; it is reset to 0 iff
``mean > max_p_normal``.
"""
import functools

import numpy as np
import scipy.sparse as sp

import _states_oracle as so
from _tsne_oracle import exp_

MAX_WINDOWS = 4096  # ICV_POSTERIOR_MAX_WINDOWS of include/infercnv_hip.h
TWO40 = 1099511627776.0
# windows per chromosome of a 1 802-window genome in proportion to the human autosomes + X
LENGTHS_1802 = (148, 144, 117, 114, 108, 102, 94, 86, 83, 79, 81, 79, 68, 63, 61, 54, 49, 48, 35, 38, 28, 30, 93)
assert sum(LENGTHS_1802) == 1802 and len(LENGTHS_1802) == 23
# The planted case of the chain cnv_states -> cnv_posteriors -> cnv_states_filter -> cnv_segments.  The calls and the
# posteriors come from the same model, so a run that Viterbi calls rarely has a mean P(neutral) above 0.5: no seed of
# 0 .. 13 loses a segment at the default threshold.  At 0.3 this seed loses two blips of 2 and 3 windows (means 0.46 and
# 0.33) and keeps every planted segment of >= 10 windows (the largest mean of those is 0.26);
# test_posterior_oracle.py checks that.
CHAIN_SEED, CHAIN_MAX_P_NORMAL = 3, 0.3


# ---- posteriors ------------------------------------------------------------------------------------------------------------
def scalars(sigma, switch_prob):
    """(h, ps, pw) of rule 1."""
    return 1.0 / (2.0 * sigma * sigma), 1.0 - switch_prob, switch_prob / 2.0


def emissions(x, a, h):
    """rule 2: [b(0), b(1), b(2)] of a float64 vector of values."""
    e = []
    for mu in (-a, 0.0, a):
        t = x - mu
        e.append(-(t * t) * h)
    m = np.maximum(np.maximum(e[0], e[1]), e[2])
    return [exp_(v - m) for v in e]


def _mix(y, k0, k1, k2):
    return ((y[0] * k0) + (y[1] * k1)) + (y[2] * k2)


def chain(xs, a, h, ps, pw):
    """rules 2-5 on one chromosome of many cells: xs float64 (n, T) -> gamma float64 (3, n, T)."""
    xs = np.asarray(xs, dtype=np.float64)
    n, T = xs.shape
    b = [emissions(xs[:, t], a, h) for t in range(T)]
    al, cs = [], []
    for t in range(T):
        if t == 0:
            u = list(b[0])
        else:
            prev = al[-1]
            pred = [_mix(prev, ps, pw, pw), _mix(prev, pw, ps, pw), _mix(prev, pw, pw, ps)]
            u = [pred[s] * b[t][s] for s in range(3)]
        c = (u[0] + u[1]) + u[2]
        al.append([u[s] / c for s in range(3)])
        cs.append(c)
    gamma = np.empty((3, n, T), dtype=np.float64)
    be = [np.ones(n), np.ones(n), np.ones(n)]
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            g = [b[t + 1][s] * be[s] for s in range(3)]
            v = [((ps * g[0]) + (pw * g[1])) + (pw * g[2]), ((pw * g[0]) + (ps * g[1])) + (pw * g[2]),
                 ((pw * g[0]) + (pw * g[1])) + (ps * g[2])]
            be = [v[r] / cs[t + 1] for r in range(3)]
        w = [al[t][s] * be[s] for s in range(3)]
        z = (w[0] + w[1]) + w[2]
        for s in range(3):
            gamma[s, :, t] = w[s] / z
    return gamma


def cnv_posteriors(x, chr_pos, amplitude=None, sigma=None, switch_prob=None, bounds=None):
    """(loss, neutral, gain float64 n x W, params dict); a None resolves as in ``_states_oracle.cnv_states``."""
    x = so.canonical(x)
    n, w = x.shape
    if sigma is None:
        sigma = so.default_sigma(x)
    if amplitude is None:
        amplitude = 2.0 * sigma
    if switch_prob is None:
        switch_prob = 1e-3
    params = {"amplitude": float(amplitude), "sigma": float(sigma), "switch_prob": float(switch_prob)}
    if sigma == 0.0:
        return np.zeros((n, w)), np.ones((n, w)), np.zeros((n, w)), params
    so.check_emissions(x, float(amplitude), float(sigma), "cnv_posteriors")
    h, ps, pw = scalars(float(sigma), float(switch_prob))
    dense = x.toarray()
    out = np.zeros((3, n, w), dtype=np.float64)
    out[1] = 1.0
    edges = [int(v) for v in bounds] if bounds is not None else so.bounds(chr_pos, w)
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 > s0:
                out[:, :, s0:s1] = chain(dense[:, s0:s1], float(amplitude), h, ps, pw)
    return out[0], out[1], out[2], params


# ---- filter ----------------------------------------------------------------------------------------------------------------
def runs(row, edges):
    """The runs of one row of calls: list of (start, end) with end exclusive, by start."""
    out = []
    row = np.asarray(row).tolist()
    for s0, s1 in zip(edges[:-1], edges[1:]):
        t = s0
        while t < s1:
            if row[t] == 0:
                t += 1
                continue
            e = t + 1
            while e < s1 and row[e] == row[t]:
                e += 1
            out.append((t, e))
            t = e
    return out


FILTER_VARIANTS = ("drop_first", "drop_first_sum", "drop_64", "drop_64_sum", "half_up", "truncate", "float_sum")


def _truncated_float(total):
    """A non-negative Python integer converted to float64 by truncation (not the filter's rule 2)."""
    shift = max(total.bit_length() - 53, 0)
    return float((total >> shift) << shift)


def _variant_mean(variant, q_row, p_row, s, e):
    """The mean of the run [s, e) under a deviation from the filter's rules (never the contract):
    drop_first / drop_64 lose the run's first window / every window at a multiple of 64 from the sum and the count,
    drop_first_sum / drop_64_sum from the sum alone; half_up rounds p 2^40 half up; truncate converts the integer sum to
    float64 by truncation; float_sum divides the sequential float64 sum of p by the length."""
    if variant == "float_sum":
        total = 0.0
        for v in p_row[s:e]:
            total = total + v
        return total / float(e - s)
    if variant == "half_up":
        return float(sum(int(np.floor(v * TWO40 + 0.5)) for v in p_row[s:e])) / (float(e - s) * TWO40)
    if variant == "truncate":
        return _truncated_float(sum(q_row[s:e])) / (float(e - s) * TWO40)
    lost = [s] if variant.startswith("drop_first") else [t for t in range(s, e) if t % 64 == 0]
    total = sum(q_row[s:e]) - sum(q_row[t] for t in lost)
    count = e - s if variant.endswith("_sum") else e - s - len(lost)
    return float(total) / (float(count) * TWO40) if count else 0.0


def states_filter(states, p_neutral, chr_pos, max_p_normal=0.5, variant=None):
    """(filtered int8 n x W, fraction float64 n, removed int32 n).  ``variant`` names one of FILTER_VARIANTS: a
    deviation from the rules that the tests show to be visible on the crafted cases."""
    assert variant is None or variant in FILTER_VARIANTS
    states = np.asarray(states)
    p = np.asarray(p_neutral, dtype=np.float64)
    if ((states < -1) | (states > 1)).any():
        raise ValueError("a call other than -1, 0 and +1")
    if not ((p >= 0.0) & (p <= 1.0)).all():
        raise ValueError("a posterior that is not a number in [0, 1]")
    n, w = states.shape
    q = np.rint(p * TWO40).astype(np.int64)
    edges = so.bounds(chr_pos, w)
    out = states.astype(np.int8).copy()
    removed = np.zeros(n, dtype=np.int32)
    for i in range(n):
        for s, e in runs(states[i], edges):
            if variant is None:
                total = sum(q[i, s:e].tolist())  # a Python integer
                mean = float(total) / (float(e - s) * TWO40)
            else:
                mean = _variant_mean(variant, q[i].tolist(), p[i].tolist(), s, e)
            if mean > max_p_normal:
                out[i, s:e] = 0
                removed[i] += 1
    return out, (out != 0).sum(axis=1).astype(np.float64) / float(w), removed


# ---- cases -----------------------------------------------------------------------------------------------------------------
def outliers():
    """Values 50 sigma from 0 under an amplitude of 20 sigma: e_gain - e_neutral = (2 x a - a a) h = 800 > 708, so the
    other two b are exactly 0 and the posteriors of those windows are exactly 0.0 and 1.0."""
    base = so.planted(8, [30, 2, 19], 31)
    dense = base["x"].toarray()
    sigma = 0.1
    dense[0, 4] = 50 * sigma
    dense[1, 29] = -50 * sigma  # the last window of a chromosome
    dense[2, 30] = 50 * sigma   # the first window of a chromosome of two
    dense[3, 10:13] = 50 * sigma
    dense[3, 13] = -50 * sigma  # the chain meets a state it gave probability 0
    base["x"] = sp.csr_matrix(dense)
    base["kwargs"] = {"sigma": sigma, "amplitude": 20 * sigma, "switch_prob": 1e-3}
    return base


CUTOFF_LENGTHS = (9, 1, 7, 1, 5)
CUTOFF_VALUES = (88.625, 88.75, 88.875)  # e_neutral - e_gain = -707, -708 (ts_exp's last non-zero argument) and -709
CUTOFF_PROBES = (0, 13, 22, 9)  # the first window of a chromosome, a middle one, the last one, a one-window chromosome
CUTOFF_KWARGS = {"sigma": 0.25, "amplitude": 0.5, "switch_prob": 1e-3}  # h = 8.0: every emission is exact


def exp_cutoff():
    """The arguments of ts_exp on its cutoff and on either side of it.  With h = 8 and a = 1/2 a value x has
    e_neutral - e_gain = 4 - 8 x: -707, -708 and -709 for the three CUTOFF_VALUES, the last of which ts_exp maps to 0.0.
    Rows 0-5: one value (+ and - of each) at the CUTOFF_PROBES windows among windows of the same sign's amplitude, where
    the chain leaves P(neutral) at b(neutral) times at most one; rows 6-11: the same among windows that are not stored
    (pred b goes subnormal next to a neutral neighbour); then extremes of both signs side by side, and noise.  Every value
    is a float32 number.  dict(x, chr_pos, kwargs, probes=[(row, window, |value|)])."""
    a = CUTOFF_KWARGS["amplitude"]
    w = sum(CUTOFF_LENGTHS)
    rows, probes = [], []
    for background in (a, 0.0):
        for v in CUTOFF_VALUES:
            for sign in (1.0, -1.0):
                row = np.full(w, sign * background)
                row[list(CUTOFF_PROBES)] = sign * v
                if background:
                    probes.extend((len(rows), t, v) for t in CUTOFF_PROBES)
                rows.append(row)
    row = np.zeros(w)
    row[0:6] = [88.875, -88.875, 88.75, -88.75, 88.625, -88.625]  # the chain meets a state it gave probability 0
    row[10:14] = [88.75, 88.75, 88.875, 88.875]
    row[18:23] = [-88.625, 0.25, -88.75, -0.25, -88.875]
    rows.append(row)
    rng = np.random.default_rng(41)
    for v in CUTOFF_VALUES:
        row = rng.normal(0.0, 0.25, size=w).astype(np.float32).astype(np.float64)
        row[rng.random(w) < 0.4] = 0.0
        row[rng.integers(0, w, size=3)] = [v, -v, v]
        rows.append(row)
    dense = np.vstack(rows)
    assert np.array_equal(dense, dense.astype(np.float32).astype(np.float64))
    return {"x": sp.csr_matrix(dense), "chr_pos": so.chr_pos_of(CUTOFF_LENGTHS), "kwargs": dict(CUTOFF_KWARGS),
            "probes": probes}


def _cases():
    rng = np.random.default_rng(11)
    many65 = rng.integers(1, 7, size=65).tolist()
    many130 = rng.integers(1, 7, size=130).tolist()
    return {
        "one_window": lambda: so.planted(3, [1], 2, keep=0.5),
        "short_chromosomes": lambda: so.planted(9, [1, 2, 3, 30, 3, 2, 1, 41, 1], 3),  # W = 84
        "odd_width": lambda: so.planted(5, [37, 64, 29], 12),  # W = 130: no multiple of 4 or 64
        "chromosomes_65": lambda: so.planted(7, many65, 4),
        "chromosomes_130": lambda: so.planted(6, many130, 5),
        "max_windows": lambda: so.planted(3, [MAX_WINDOWS], 6),
        "planted300": lambda: so.planted(300, LENGTHS_1802, CHAIN_SEED),
        "full_and_empty": so.full_and_empty,
        "outliers": outliers,
        "exp_cutoff": exp_cutoff,
        "switch_0.3": lambda: dict(so.planted(40, [25, 1, 2, 40, 13], 14), kwargs={"switch_prob": 0.3}),
        "switch_1e-12": lambda: dict(so.planted(40, [25, 1, 2, 40, 13], 14), kwargs={"switch_prob": 1e-12}),
        "switch_1e-3": lambda: dict(so.planted(40, [25, 1, 2, 40, 13], 14), kwargs={"switch_prob": 1e-3}),
    }


CASE_NAMES = tuple(_cases())


@functools.lru_cache(maxsize=None)
def case(name):
    """The named case with its expected output, computed once: dict(x, chr_pos, kwargs, loss, neutral, gain, params)."""
    c = _cases()[name]()
    c["loss"], c["neutral"], c["gain"], c["params"] = cnv_posteriors(c["x"], c["chr_pos"], **c["kwargs"])
    for k in ("loss", "neutral", "gain"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def chain_case():
    """The oracle chain on the planted case: dict(x, chr_pos, truth, states, fraction, params, neutral, filtered,
    filtered_fraction, removed)."""
    c = dict(case("planted300"))
    c["states"], c["fraction"], params = so.cnv_states(c["x"], c["chr_pos"])
    assert params == c["params"]
    c["filtered"], c["filtered_fraction"], c["removed"] = states_filter(c["states"], c["neutral"], c["chr_pos"],
                                                                        CHAIN_MAX_P_NORMAL)
    for k in ("states", "fraction", "filtered", "filtered_fraction", "removed"):
        c[k].setflags(write=False)
    return c


def planted_segments_kept(truth, calls, edges, min_windows=10):
    """(number of planted segments of >= min_windows windows, how many of them still carry a call of their sign)."""
    total = kept = 0
    for i in range(truth.shape[0]):
        for s, e in runs(truth[i], edges):
            if e - s >= min_windows:
                total += 1
                kept += bool((calls[i, s:e] == truth[i, s]).any())
    return total, kept


def crafted_filter_cases():
    """{name: dict(states int8, p float64, chr_pos, max_p_normal, want int8)}: the verdicts that a wrong comparison, a
    wrong run definition or a floating-point mean would get wrong."""
    half = np.full((1, 8), 0.5)
    ones = np.array([[0, 1, 1, 1, 1, 1, 0, 0]], dtype=np.int8)
    out = {
        "mean_equal_to_the_threshold_stays": dict(states=ones, p=half, chr_pos={"a": 0}, max_p_normal=0.5, want=ones),
        "mean_2^-30_above_goes": dict(states=ones, p=half + 2.0 ** -30, chr_pos={"a": 0}, max_p_normal=0.5,
                                     want=np.zeros_like(ones)),
        "loss_then_gain_is_two_runs": dict(
            states=np.array([[-1, -1, 1, 1, 0]], dtype=np.int8), p=np.array([[0.9, 0.9, 0.1, 0.1, 0.3]]),
            chr_pos={"a": 0}, max_p_normal=0.5, want=np.array([[0, 0, 1, 1, 0]], dtype=np.int8)),
        "chromosome_boundary_cuts_a_run": dict(
            states=np.array([[1, 1, 1, 1, 1, 1]], dtype=np.int8), p=np.array([[0.9, 0.9, 0.9, 0.1, 0.1, 0.1]]),
            chr_pos={"a": 0, "b": 3}, max_p_normal=0.5, want=np.array([[0, 0, 0, 1, 1, 1]], dtype=np.int8)),
    }
    return out


def random_calls(n, lengths, seed, p_run=0.5):
    """(states int8 n x W, p float64 n x W): runs of geometric lengths, posteriors that are low, high or mixed per run."""
    rng = np.random.default_rng(seed)
    w = int(sum(lengths))
    states = np.zeros((n, w), dtype=np.int8)
    p = rng.random((n, w))
    for i in range(n):
        t = 0
        while t < w:
            length = int(rng.geometric(0.15))
            value = int(rng.integers(-1, 2)) if rng.random() < p_run else 0
            states[i, t:t + length] = value
            kind = rng.integers(0, 3)
            if kind == 0:
                p[i, t:t + length] *= 0.4
            elif kind == 1:
                p[i, t:t + length] = 0.6 + 0.4 * p[i, t:t + length]
            t += length
    return states, p


# ---- the filter at its step boundaries and integer rules -------------------------------------------------------------------
SWEEP_W = 200
SWEEP_POINTS = (0, 1, 2, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 190, 191, 192, 193, 199, 200)
SWEEP_NEIGHBOURHOODS = ("alone", "behind_other_sign", "before_same_sign_chromosome")


def _balanced_k(rng, length, target):
    """length integers in [-3, 3] that sum to target."""
    k = rng.integers(-3, 4, size=length)
    diff = int(target - k.sum())
    for i in rng.permutation(length):
        if diff == 0:
            break
        step = int(np.clip(k[i] + diff, -3, 3)) - int(k[i])
        k[i] += step
        diff -= step
    assert diff == 0 and np.abs(k).max() <= 3
    return k


def _sweep_rows(rng, pairs, neighbourhood):
    n = len(pairs)
    states = np.zeros((n, SWEEP_W), dtype=np.int8)
    k = rng.integers(-3, 4, size=(n, SWEEP_W))
    for i, (s, e) in enumerate(pairs):
        sign = 1 if i % 2 else -1
        goes = (i // 2) % 2  # sum(k) = 1: the mean is above 0.5 by 2^-40 / L; sum(k) = 0: it is 0.5 and the run stays
        states[i, s:e] = sign
        k[i, s:e] = _balanced_k(rng, e - s, goes)
        if neighbourhood == "behind_other_sign":
            states[i, max(0, s - (1, 2, 65, 130)[i % 4]):s] = -sign
        elif neighbourhood == "before_same_sign_chromosome":
            e2 = min(SWEEP_W, e + (1, 2, 65, 130)[i % 4])
            states[i, e:e2] = sign
            k[i, e:e2] = _balanced_k(rng, e2 - e, 1 - goes)  # one run in place of the two would have another verdict
    return states, 0.5 + k * 2.0 ** -40


@functools.lru_cache(maxsize=None)
def sweep_cases(neighbourhood):
    """The step-boundary sweep: every run [s, e) with s < e from SWEEP_POINTS in one row of 200 windows, the posteriors
    0.5 + k_t 2^-40 with integer k_t in [-3, 3], so that at max_p_normal = 0.5 the verdict of a run is sum(k_t) > 0 and
    the run's sum is 0 or 1: a window lost or counted twice flips it.  List of dict(states, p, chr_pos, main=[(s, e)],
    max_p_normal); the third neighbourhood is one call per e, whose chromosome start it needs."""
    assert neighbourhood in SWEEP_NEIGHBOURHOODS
    rng = np.random.default_rng(SWEEP_NEIGHBOURHOODS.index(neighbourhood) + 100)
    pairs = [(s, e) for s in SWEEP_POINTS for e in SWEEP_POINTS if s < e]
    if neighbourhood == "behind_other_sign":
        pairs = [(s, e) for s, e in pairs if s > 0]
    groups = [({"a": 0}, pairs)]
    if neighbourhood == "before_same_sign_chromosome":
        groups = [({"a": 0, "b": end}, [(s, e) for s, e in pairs if e == end]) for end in SWEEP_POINTS[1:-1]]
    out = []
    for chr_pos, sel in groups:
        states, p = _sweep_rows(rng, sel, neighbourhood)
        out.append({"states": states, "p": p, "chr_pos": chr_pos, "main": sel, "max_p_normal": 0.5})
    return out


def half_integer_case():
    """p = (2 j + 1) / 2^41, so p 2^40 = j + 1/2 exactly.  Row 0: runs of even j = 2^39 + d with sum(d) = 0: rounding
    half to even keeps j, the mean is exactly 0.5 and the run stays; rounding half up adds one per window and it goes.
    Row 1: runs of odd j = 2^39 - 1 + d (d even, sum(d) = 0): half to even and half up both give j + 1, the mean is
    exactly 0.5 and the run stays; rounding half down would leave it below.  Row 2: odd j whose sum is 2 above: the run
    goes.  dict(states, p, chr_pos, max_p_normal)."""
    rng = np.random.default_rng(77)
    lengths = (1, 2, 3, 63, 64, 65, 130)
    w = sum(lengths) + len(lengths)
    states = np.zeros((3, w), dtype=np.int8)
    j = np.full((3, w), 2 ** 39, dtype=np.int64)
    t = 0
    for n, length in enumerate(lengths):
        d = 2 * _balanced_k(rng, length, 0)
        states[:, t:t + length] = 1 if n % 2 else -1
        j[0, t:t + length] = 2 ** 39 + d
        j[1, t:t + length] = 2 ** 39 - 1 + d
        j[2, t:t + length] = 2 ** 39 - 1 + d
        j[2, t] += 2
        t += length + 1
    p = (2 * j + 1).astype(np.float64) / 2.0 ** 41
    assert np.array_equal(p * 2.0 ** 41, (2 * j + 1).astype(np.float64))
    return {"states": states, "p": p, "chr_pos": {"a": 0}, "max_p_normal": 0.5}


BIG_W = 20000
BIG_RUNS = ((1, 16386), (3000, 19999), (0, 20000))  # 16 385, 16 999 and 20 000 windows: sums above 2^53


@functools.lru_cache(maxsize=None)
def big_sum_case():
    """Runs whose integer sum S is above 2^54, where float64 holds multiples of 4 only: p = 1 - k_t 2^-40 with k_t in
    [0, 7] and S = 1, 2, 3 modulo 4 in the three rows, so the int64 -> float64 conversion of rule 2 rounds down, to even
    and up.  dict(states, p, chr_pos, means): every row is run at max_p_normal = its own mean (the run stays) and at the
    float64 below it (the run goes)."""
    rng = np.random.default_rng(53)
    states = np.zeros((3, BIG_W), dtype=np.int8)
    k = rng.integers(0, 8, size=(3, BIG_W))
    means = []
    for i, (s, e) in enumerate(BIG_RUNS):
        states[i, s:e] = 1 if i % 2 else -1
        total = (e - s) * 2 ** 40 - int(k[i, s:e].sum())
        while total % 4 != i + 1:  # one more unit of k: the sum falls by one
            t = int(rng.integers(s, e))
            if k[i, t] < 7:
                k[i, t] += 1
                total -= 1
        assert total > 2 ** 54 and total == (e - s) * 2 ** 40 - int(k[i, s:e].sum())
        means.append(float(total) / (float(e - s) * TWO40))
    p = 1.0 - k * 2.0 ** -40
    assert np.array_equal((1.0 - p) * TWO40, k.astype(np.float64)) and p.max() <= 1.0
    p.setflags(write=False)
    states.setflags(write=False)
    return {"states": states, "p": p, "chr_pos": {"a": 0}, "means": means}


def own_mean_cases():
    """50 runs of random posteriors, lengths 1 .. 130, each a call of its own: list of dict(states 1 x 136, p, chr_pos,
    thresholds = (the float64 below the run's mean, the mean, the float64 above it))."""
    rng = np.random.default_rng(50)
    out = []
    for n in range(50):
        length = int(rng.integers(1, 131)) if n >= 6 else (1, 2, 63, 64, 65, 130)[n]
        w = 136
        s = int(rng.integers(0, w - length + 1))
        states = np.zeros((1, w), dtype=np.int8)
        states[0, s:s + length] = 1 if n % 2 else -1
        p = rng.random((1, w))
        total = sum(np.rint(p[0, s:s + length] * TWO40).astype(np.int64).tolist())
        mean = float(total) / (float(length) * TWO40)
        out.append({"states": states, "p": p, "chr_pos": {"a": 0},
                    "thresholds": (float(np.nextafter(mean, 0.0)), mean, float(np.nextafter(mean, 2.0)))})
    return out

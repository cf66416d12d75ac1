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


def cnv_posteriors(x, chr_pos, amplitude=None, sigma=None, switch_prob=None):
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
    h, ps, pw = scalars(float(sigma), float(switch_prob))
    dense = x.toarray()
    out = np.empty((3, n, w), dtype=np.float64)
    edges = so.bounds(chr_pos, w)
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
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


def states_filter(states, p_neutral, chr_pos, max_p_normal=0.5):
    """(filtered int8 n x W, fraction float64 n, removed int32 n)."""
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
            total = sum(q[i, s:e].tolist())  # a Python integer
            mean = float(total) / (float(e - s) * TWO40)
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

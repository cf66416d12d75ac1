"""Numpy oracle of tl.cnv_copy_states_fit: Baum-Welch for the amplitude, sigma and switch_prob of the
K-state model of tl.cnv_copy_states on a lattice of levels, ``levels = [float(k) * amplitude for k in steps]``.

E-step.  All arithmetic is IEEE float64 without fused multiply-add, one numpy operation per written operation (the cells
are the vector axis, the windows and the states explicit loops).  Rules 1-6 of ``_copy_posterior_oracle`` give ``b``,
``al_t``, ``c_t``, ``be_t``, ``w``, ``z_t`` and ``gamma_t``.  Per cell and chromosome of T >= 1 windows 2K + 1 sums start
at ``0.0`` and take their terms for t = T-1 down to 0:

* ``N_s += gamma_t(s)`` for s = 0 .. K-1
* ``M_s += gamma_t(s) * x_t`` (the product rounded before the add)
* for t <= T-2, with ``g(s) = b_{t+1}(s) * be_{t+1}(s)``, ``m(s) = (al_t(s) * ps) * g(s)`` and
  ``st = (..(m(0) + m(1)) + ..) + m(K-1)``: ``S += (st / c_{t+1}) / z_t``

The cell's sums start at ``0.0`` and add the chromosome sums in ascending chromosome order; a chromosome without windows
adds nothing, nor does a window that no chromosome covers.  ``stats[i] = (N_0 .. N_{K-1}, M_0 .. M_{K-1}, S)``.

M-step, in Python floats.  ``Ns_s = fsum(N_s of the cells)``, ``Ms_s`` and ``Ss`` likewise, ``Qs = fsum(rowsq_i)``;
``N = float(n) float(W)``, ``NT = n sum(max(T_c - 1, 0))``; ``k_s = float(steps[s])``.

* amplitude: ``num = fsum(k_s Ms_s)``, ``den = fsum((k_s k_s) Ns_s)``; if fitted and ``num > 0`` and ``den > 0``:
  ``a' = num / den``; otherwise ``a' = a``.  ``mu'_s = k_s a'``.
* sigma (if fitted): ``var = ((Qs - 2.0 fsum(mu'_s Ms_s)) + fsum((mu'_s mu'_s) Ns_s)) / N``, ``sigma' = sqrt(var)``.
* switch_prob (if fitted and ``NT > 0``): ``p' = min(max(1.0 - Ss / NT, 1e-9), 0.5)``.

A step whose ``var`` is not finite or not ``> 0`` (or whose ``a'`` or ``1 / (2 sigma' sigma')`` is not finite) is
degenerate: the fit stops with the parameters of the iteration before.  ``delta`` is the largest ``|new - old| / old``
over the fitted parameters; ``delta <= tol`` ends the loop converged.

Start values.  ``sigma=None``: the difference-based estimate of ``_changepoint_oracle.default_sigma``; where that is 0
(no chromosome has two windows, or all differences are 0) the root mean square of ``_states_oracle.default_sigma``.
``amplitude=None``: ``2 sigma``.  ``switch_prob=None``: ``1e-3``.  Start values whose emission overflows (rule 6 of
``_copy_states_oracle`` under ``max(|mu[0]|, |mu[-1]|)``) are a ``ValueError``.
"""
import math

import numpy as np

import _changepoint_oracle as cho
import _copy_posterior_oracle as cpo
import _copy_states_oracle as co
import _states_oracle as so

NAMES = ("amplitude", "sigma", "switch_prob")
P_MIN, P_MAX = 1e-9, 0.5
LDS_BYTES = cpo.LDS_BYTES

# The planted case of DESIGN.md 4.22 (_copy_states_oracle.planted_levels), seeds 0-4, all defaults: what this oracle's fit
# gives.  test_copy_fit_oracle.py recomputes every figure.
PLANTED_WRONG = (15, 22, 16, 25, 21)  # wrong calls of 3 120 under the fitted params
PLANTED_AMPLITUDE = (0.2992507335729144, 0.29890804659073905, 0.299430360740068, 0.29849558059057024, 0.2973459376866586)
PLANTED_SIGMA = (0.10048145350174774, 0.09974594886597467, 0.10017724382141012, 0.10097639286755848, 0.09859777434868923)
PLANTED_N_ITER = (4, 5, 5, 5, 4)
PLANTED_RMS_START_WRONG = (1088, 1076, 1092, 1077, 1064)  # calls under sigma = RMS, amplitude = 2 RMS, unfitted


def lds_bytes(w, k, n_chr):
    """ICV_COPY_POSTERIOR_STATS_LDS of include/infercnv_hip.h."""
    return 8 * ((k + 1) * w + (2 * k + 1) * n_chr)


def max_windows(k, n_chr):
    """ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS of include/infercnv_hip.h."""
    return max(LDS_BYTES - 8 * (2 * k + 1) * n_chr, 0) // (8 * (k + 1))


# ---- E-step ----------------------------------------------------------------------------------------------------------------
def _forward(xs, mu, h, ps, pw):
    """rules 2-3 on one chromosome of many cells: (b, al, cs), lists over the windows."""
    T = xs.shape[1]
    k = len(mu)
    b = [cpo.emissions(xs[:, t], mu, h) for t in range(T)]
    al, cs = [], []
    for t in range(T):
        if t == 0:
            u = list(b[0])
        else:
            pred = cpo._pred(al[-1], ps, pw, None)
            u = [pred[s] * b[t][s] for s in range(k)]
        c = cpo._sum(u)
        al.append([u[s] / c for s in range(k)])
        cs.append(c)
    return b, al, cs


def chain_stats(xs, mu, h, ps, pw):
    """The sums of one chromosome of many cells: xs float64 (n, T), T >= 1 -> (N, M, S): two lists of K float64 (n,)
    vectors and one vector."""
    xs = np.asarray(xs, dtype=np.float64)
    n, T = xs.shape
    k = len(mu)
    b, al, cs = _forward(xs, mu, h, ps, pw)
    N, M, S = [np.zeros(n) for _ in range(k)], [np.zeros(n) for _ in range(k)], np.zeros(n)
    be = [np.ones(n) for _ in range(k)]
    g = None
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            g = [b[t + 1][s] * be[s] for s in range(k)]
            v = [cpo._mix(g, [ps if r == s else pw for s in range(k)], None) for r in range(k)]
            be = [v[r] / cs[t + 1] for r in range(k)]
        w = [al[t][s] * be[s] for s in range(k)]
        z = cpo._sum(w)
        for s in range(k):
            gamma = w[s] / z
            N[s] = N[s] + gamma
            M[s] = M[s] + gamma * xs[:, t]
        if t < T - 1:
            m = [(al[t][s] * ps) * g[s] for s in range(k)]
            st = cpo._sum(m)
            S = S + (st / cs[t + 1]) / z
    return N, M, S


def stats(x, chr_pos, levels, sigma, switch_prob, bounds=None):
    """The n x (2K + 1) float64 array of the sums per cell; ``bounds=`` takes the kernel's own ``chr_start`` array in place
    of ``chr_pos`` (a chromosome with ``s1 <= s0`` adds nothing, nor does a window that no chromosome covers)."""
    x = so.canonical(x)
    n, w = x.shape
    mu = [float(v) for v in levels]
    k = len(mu)
    h, ps, pw = cpo.scalars(float(sigma), float(switch_prob), k)
    dense = x.toarray()
    out = np.zeros((n, 2 * k + 1), dtype=np.float64)
    edges = [int(v) for v in bounds] if bounds is not None else so.bounds(chr_pos, w)
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 <= s0:
                continue
            N, M, S = chain_stats(dense[:, s0:s1], mu, h, ps, pw)
            for s in range(k):
                out[:, s] = out[:, s] + N[s]
                out[:, k + s] = out[:, k + s] + M[s]
            out[:, 2 * k] = out[:, 2 * k] + S
    return out


# ---- M-step ----------------------------------------------------------------------------------------------------------------
def check_steps(steps):
    """The tuple of K ints: strictly ascending integers containing 0, 2 <= K <= 8."""
    out = []
    for v in steps:
        if isinstance(v, bool) or int(v) != v:
            raise ValueError(f"cnv_copy_states_fit: step {v!r} is not an integer")
        out.append(int(v))
    if not co.MIN_STATES <= len(out) <= co.MAX_STATES:
        raise ValueError(f"cnv_copy_states_fit: {len(out)} states")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("cnv_copy_states_fit: the steps do not ascend strictly")
    if 0 not in out:
        raise ValueError("cnv_copy_states_fit: no step is 0")
    return tuple(out)


def levels_of(steps, amplitude):
    return [float(k) * amplitude for k in steps]


def m_step(Ns, Ms, Ss, Qs, N, NT, steps, a, sigma, p, fit):
    """(a', sigma', p'), or None for a degenerate step.  Ns, Ms: lists of K floats."""
    ks = [float(k) for k in steps]
    num = math.fsum(ks[s] * Ms[s] for s in range(len(ks)))
    den = math.fsum((ks[s] * ks[s]) * Ns[s] for s in range(len(ks)))
    if "amplitude" in fit and num > 0 and den > 0:
        a = num / den
    mu = [k * a for k in ks]
    if "sigma" in fit:
        var = ((Qs - 2.0 * math.fsum(mu[s] * Ms[s] for s in range(len(ks))))
               + math.fsum((mu[s] * mu[s]) * Ns[s] for s in range(len(ks)))) / N
        if not (math.isfinite(var) and var > 0):
            return None
        sigma = math.sqrt(var)
    if "switch_prob" in fit and NT > 0:
        p = min(max(1.0 - Ss / NT, P_MIN), P_MAX)
    try:
        ok = math.isfinite(a) and math.isfinite(1.0 / (2.0 * sigma * sigma))
    except ZeroDivisionError:
        ok = False
    return (a, sigma, p) if ok else None


def _dict(a, sigma, p):
    return {"amplitude": float(a), "sigma": float(sigma), "switch_prob": float(p)}


def start_sigma(x, chr_pos):
    """The default start value of sigma; x canonical."""
    s = cho.default_sigma(x, chr_pos)
    return s if s > 0.0 else so.default_sigma(x)


def cnv_copy_states_fit(x, chr_pos, steps=None, amplitude=None, sigma=None, switch_prob=None, fit=("amplitude", "sigma"),
                        max_iter=25, tol=1e-4):
    """dict(params={levels, sigma, switch_prob}, amplitude, steps, history, n_iter, converged, fit, and
    stopped="degenerate" where the fit ended so)."""
    fit = [k for k in NAMES if k in fit]
    steps = check_steps(co.DEFAULT_STEPS if steps is None else steps)
    x = so.canonical(x)
    n, w = x.shape
    if sigma is None:
        sigma = start_sigma(x, chr_pos)
    if amplitude is None:
        amplitude = 2.0 * sigma
    if switch_prob is None:
        switch_prob = 1e-3
    cur = (float(amplitude), float(sigma), float(switch_prob))

    def result(cur, **more):
        return dict({"params": {"levels": levels_of(steps, cur[0]), "sigma": cur[1], "switch_prob": cur[2]},
                     "amplitude": cur[0], "steps": list(steps)}, **more)

    out = {"history": [_dict(*cur)], "n_iter": 0, "converged": False, "fit": fit}
    if cur[1] == 0.0:
        return result(cur, **out)
    co.check_emissions(x, levels_of(steps, cur[0]), cur[1])  # the start values; later steps end as degenerate ones
    k = len(steps)
    Qs, N, NT = math.fsum(so.rowsq(x)), float(n) * float(w), _n_steps(chr_pos, n, w)
    for _ in range(max_iter):
        s = stats(x, chr_pos, levels_of(steps, cur[0]), cur[1], cur[2])
        out["n_iter"] += 1
        sums = [math.fsum(s[:, j].tolist()) for j in range(2 * k + 1)]
        new = m_step(sums[:k], sums[k:2 * k], sums[2 * k], Qs, N, NT, steps, *cur, fit)
        if new is None:
            out["stopped"] = "degenerate"
            break
        delta = max(abs(new[j] - cur[j]) / cur[j] for j in range(3) if NAMES[j] in fit)
        cur = new
        out["history"].append(_dict(*cur))
        if delta <= tol:
            out["converged"] = True
            break
    return result(cur, **out)


def _n_steps(chr_pos, n, w):
    """NT: the number of steps t -> t + 1 inside the chromosomes of all cells."""
    edges = so.bounds(chr_pos, w)
    return n * sum(max(s1 - s0 - 1, 0) for s0, s1 in zip(edges[:-1], edges[1:]))


# ---- the likelihood the fit climbs (for one property; never compared bitwise) -----------------------------------------------
def loglik(x, chr_pos, levels, sigma, switch_prob):
    """log P(x | levels, sigma, switch_prob) of the whole matrix under the model: uniform start, chains per chromosome."""
    mu = [float(v) for v in levels]
    k = len(mu)
    x = so.canonical(x)
    n, w = x.shape
    h, ps, pw = cpo.scalars(float(sigma), float(switch_prob), k)
    dense = x.toarray()
    edges = so.bounds(chr_pos, w)
    total = 0.0
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 <= s0:
                continue
            xs = dense[:, s0:s1]
            _, _, cs = _forward(xs, mu, h, ps, pw)
            total += float(sum(np.log(c).sum() for c in cs))
            e = np.stack([-((xs - m) * (xs - m)) * h for m in mu])
            total += float(e.max(axis=0).sum())  # the maxima rule 2 subtracted
            total -= n * math.log(float(k))  # the uniform start
    return total - float(n) * float(w) * math.log(sigma * math.sqrt(2.0 * math.pi))

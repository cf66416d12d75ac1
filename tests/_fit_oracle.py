"""Numpy oracle of tl.cnv_states_fit: Baum-Welch for the amplitude, sigma and switch_prob of the
three-state model of tl.cnv_states.

E-step.  All arithmetic is IEEE float64 without fused multiply-add, one numpy operation per written operation (the cells
are the vector axis, the windows an explicit loop).  Rules 1-5 of ``_posterior_oracle`` give ``b``, ``al_t``, ``c_t``,
``be_t``, ``w``, ``z_t`` and ``gamma_t``.  Per cell and chromosome of T >= 1 windows three sums start at ``0.0`` and take
their terms for t = T-1 down to 0:

* ``G += (gamma_t(0) + gamma_t(2))``
* ``D += (gamma_t(2) - gamma_t(0)) * x_t``
* for t <= T-2, with ``g(s) = b_{t+1}(s) * be_{t+1}(s)``, ``m(s) = (al_t(s) * ps) * g(s)`` and
  ``st = (m(0) + m(1)) + m(2)``: ``K += (st / c_{t+1}) / z_t``

The cell's ``G``, ``D`` and ``K`` start at ``0.0`` and add the chromosome sums in ascending chromosome order; a chromosome
without windows adds nothing.

M-step, in Python floats.  ``Gs = fsum(G_i)``, ``Ds``, ``Ks`` likewise, ``Qs = fsum(rowsq_i)``; ``N = float(n) float(W)``,
``NT = n sum(max(T_c - 1, 0))``.

* amplitude (if fitted and ``Gs > 0`` and ``Ds > 0``): ``a' = Ds / Gs``; otherwise ``a' = a``.
* sigma (if fitted): ``var = ((Qs - (2.0 a') Ds) + (a' a') Gs) / N``, ``sigma' = sqrt(var)``.
* switch_prob (if fitted and ``NT > 0``): ``p' = min(max(1.0 - Ks / NT, 1e-9), 0.5)``.

A step whose ``var`` is not finite or not ``> 0`` (or whose ``a'`` or ``1 / (2 sigma' sigma')`` is not finite) is
degenerate: the fit stops with the parameters of the iteration before.  ``delta`` is the largest ``|new - old| / old``
over the fitted parameters; ``delta <= tol`` ends the loop converged.

Start values whose emission overflows (rule 6 of ``_states_oracle``) are a ``ValueError``.
"""
import math

import numpy as np
import scipy.sparse as sp

import _posterior_oracle as po
import _states_oracle as so

NAMES = ("amplitude", "sigma", "switch_prob")
P_MIN, P_MAX = 1e-9, 0.5


# ---- E-step ----------------------------------------------------------------------------------------------------------------
def _forward(xs, a, h, ps, pw):
    """rules 2-3 on one chromosome of many cells: (b, al, cs), lists over the windows."""
    T = xs.shape[1]
    b = [po.emissions(xs[:, t], a, h) for t in range(T)]
    al, cs = [], []
    for t in range(T):
        if t == 0:
            u = list(b[0])
        else:
            prev = al[-1]
            pred = [po._mix(prev, ps, pw, pw), po._mix(prev, pw, ps, pw), po._mix(prev, pw, pw, ps)]
            u = [pred[s] * b[t][s] for s in range(3)]
        c = (u[0] + u[1]) + u[2]
        al.append([u[s] / c for s in range(3)])
        cs.append(c)
    return b, al, cs


def chain_stats(xs, a, h, ps, pw):
    """The sums of one chromosome of many cells: xs float64 (n, T), T >= 1 -> (G, D, K), float64 (n,) each."""
    xs = np.asarray(xs, dtype=np.float64)
    n, T = xs.shape
    b, al, cs = _forward(xs, a, h, ps, pw)
    G, D, K = np.zeros(n), np.zeros(n), np.zeros(n)
    be = [np.ones(n), np.ones(n), np.ones(n)]
    g = None
    for t in range(T - 1, -1, -1):
        if t < T - 1:
            g = [b[t + 1][s] * be[s] for s in range(3)]
            v = [((ps * g[0]) + (pw * g[1])) + (pw * g[2]), ((pw * g[0]) + (ps * g[1])) + (pw * g[2]),
                 ((pw * g[0]) + (pw * g[1])) + (ps * g[2])]
            be = [v[r] / cs[t + 1] for r in range(3)]
        w = [al[t][s] * be[s] for s in range(3)]
        z = (w[0] + w[1]) + w[2]
        gamma0, gamma2 = w[0] / z, w[2] / z
        G = G + (gamma0 + gamma2)
        D = D + (gamma2 - gamma0) * xs[:, t]
        if t < T - 1:
            m = [(al[t][s] * ps) * g[s] for s in range(3)]
            st = (m[0] + m[1]) + m[2]
            K = K + (st / cs[t + 1]) / z
    return G, D, K


def stats(x, chr_pos, a, sigma, p, bounds=None):
    """The n x 3 float64 array of (G, D, K) per cell; ``bounds=`` takes the kernel's own ``chr_start`` array in place of
    ``chr_pos`` (a chromosome with ``s1 <= s0`` adds nothing, nor does a window that no chromosome covers)."""
    x = so.canonical(x)
    n, w = x.shape
    h, ps, pw = po.scalars(float(sigma), float(p))
    dense = x.toarray()
    out = np.zeros((n, 3), dtype=np.float64)
    edges = [int(v) for v in bounds] if bounds is not None else so.bounds(chr_pos, w)
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 <= s0:
                continue
            G, D, K = chain_stats(dense[:, s0:s1], float(a), h, ps, pw)
            out[:, 0] = out[:, 0] + G
            out[:, 1] = out[:, 1] + D
            out[:, 2] = out[:, 2] + K
    return out


# ---- M-step ----------------------------------------------------------------------------------------------------------------
def steps(chr_pos, n, w):
    """NT: the number of steps t -> t + 1 inside the chromosomes of all cells."""
    edges = so.bounds(chr_pos, w)
    return n * sum(max(s1 - s0 - 1, 0) for s0, s1 in zip(edges[:-1], edges[1:]))


def m_step(Gs, Ds, Ks, Qs, N, NT, a, sigma, p, fit):
    """(a', sigma', p'), or None for a degenerate step."""
    if "amplitude" in fit and Gs > 0 and Ds > 0:
        a = Ds / Gs
    if "sigma" in fit:
        var = ((Qs - (2.0 * a) * Ds) + (a * a) * Gs) / N
        if not (math.isfinite(var) and var > 0):
            return None
        sigma = math.sqrt(var)
    if "switch_prob" in fit and NT > 0:
        p = min(max(1.0 - Ks / NT, P_MIN), P_MAX)
    try:
        ok = math.isfinite(a) and math.isfinite(1.0 / (2.0 * sigma * sigma))
    except ZeroDivisionError:
        ok = False
    return (a, sigma, p) if ok else None


def _dict(a, sigma, p):
    return {"amplitude": float(a), "sigma": float(sigma), "switch_prob": float(p)}


def cnv_states_fit(x, chr_pos, amplitude=None, sigma=None, switch_prob=None, fit=("amplitude", "sigma"), max_iter=25,
                   tol=1e-4):
    """dict(params, history, n_iter, converged, fit, and stopped="degenerate" where the fit ended so); a None start value
    resolves as in ``_states_oracle.cnv_states``."""
    fit = [k for k in NAMES if k in fit]
    x = so.canonical(x)
    n, w = x.shape
    q = so.rowsq(x)
    if sigma is None:
        sigma = math.sqrt(math.fsum(q) / (float(n) * float(w)))
    if amplitude is None:
        amplitude = 2.0 * sigma
    if switch_prob is None:
        switch_prob = 1e-3
    cur = (float(amplitude), float(sigma), float(switch_prob))
    out = {"params": _dict(*cur), "history": [_dict(*cur)], "n_iter": 0, "converged": False, "fit": fit}
    if cur[1] == 0.0:
        return out
    so.check_emissions(x, cur[0], cur[1], "cnv_states_fit")  # the start values; later steps end as degenerate ones
    Qs, N, NT = math.fsum(q), float(n) * float(w), steps(chr_pos, n, w)
    for _ in range(max_iter):
        s = stats(x, chr_pos, *cur)
        out["n_iter"] += 1
        Gs, Ds, Ks = (math.fsum(s[:, k].tolist()) for k in range(3))
        new = m_step(Gs, Ds, Ks, Qs, N, NT, *cur, fit)
        if new is None:
            out["stopped"] = "degenerate"
            break
        delta = max(abs(new[k] - cur[k]) / cur[k] for k in range(3) if NAMES[k] in fit)
        cur = new
        out["history"].append(_dict(*cur))
        out["params"] = _dict(*cur)
        if delta <= tol:
            out["converged"] = True
            break
    return out


# ---- the likelihood the fit climbs (for one property; never compared bitwise) -----------------------------------------------
def loglik(x, chr_pos, amplitude, sigma, switch_prob):
    """log P(x | amplitude, sigma, switch_prob) of the whole matrix under the model: uniform start, chains per
    chromosome."""
    a, p = float(amplitude), float(switch_prob)
    x = so.canonical(x)
    n, w = x.shape
    h, ps, pw = po.scalars(float(sigma), float(p))
    dense = x.toarray()
    edges = so.bounds(chr_pos, w)
    total = 0.0
    with np.errstate(all="ignore"):
        for s0, s1 in zip(edges[:-1], edges[1:]):
            if s1 <= s0:
                continue
            xs = dense[:, s0:s1]
            _, _, cs = _forward(xs, float(a), h, ps, pw)
            total += float(sum(np.log(c).sum() for c in cs))
            e = np.stack([-((xs - mu) * (xs - mu)) * h for mu in (-a, 0.0, a)])
            total += float(e.max(axis=0).sum())  # the maxima rule 2 subtracted
            total -= n * math.log(3.0)  # the uniform start
    return total - float(n) * float(w) * math.log(sigma * math.sqrt(2.0 * math.pi))


# ---- cases -----------------------------------------------------------------------------------------------------------------
def degenerate_case():
    """Values exactly 0, +a and -a with a start sigma so small that every other emission underflows to 0: the posteriors
    are exactly 0 and 1, a' = a and the updated variance is exactly 0."""
    a = 0.5
    rng = np.random.default_rng(8)
    dense = rng.choice([0.0, a, -a], size=(6, 25), p=[0.6, 0.2, 0.2])
    return sp.csr_matrix(dense), {"c": 0, "d": 11}, {"amplitude": a, "sigma": 1e-3}

"""tl.cnv_copy_states_fit: Baum-Welch fit of the parameters of ``tl.cnv_copy_states`` (no counterpart in the reference).

``tl.cnv_copy_states`` and its siblings run on a rule of thumb: ``sigma`` is the root mean square of the whole matrix,
altered windows included, and the step between the levels is ``2 * sigma``.  The multi-level model is far more sensitive
to that than the three-state one, because a wrong step moves every level.  Here expectation-maximisation fits the step
(``amplitude``) of a lattice of levels, ``levels = [k * amplitude for k in steps]``, together with ``sigma`` and, on
request, ``switch_prob``.  The E-step is a forward-backward pass along every chromosome of every cell on the GPU that
leaves 2K + 1 sums per cell; the M-step is a few scalar operations on the host.  Both follow the written contract of
DESIGN.md 4.24 (float64, a fixed order), so the fit is a pure function of (matrix, chr_pos, steps, start values, fit,
max_iter, tol) and equals ``tests/_copy_fit_oracle.py`` bit for bit.
"""
from __future__ import annotations

import math
import time
import warnings

from .. import _engine, _lib
from ._changepoints import default_sigma
from ._fit import _NAMES, _P_MAX, _P_MIN, _as_dict, _fit_options
from ._hmm import DEFAULT_STEPS, MAX_STATES, MIN_STATES, check_emissions, resolve

_WHO = "tl.cnv_copy_states_fit"


def check_steps(steps, who=_WHO):
    """The tuple of K ints; ``ValueError`` unless ``steps`` are K integers, 2 <= K <= 8, strictly ascending, one of them
    0 (the neutral state)."""
    try:
        raw = list(steps)
    except TypeError:
        raise ValueError(f"{who}: steps={steps!r} must be a sequence of integers") from None
    out = []
    for v in raw:
        try:
            k = int(v)
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"{who}: steps={steps!r} must be integers") from None
        if isinstance(v, bool) or k != v:
            raise ValueError(f"{who}: steps={steps!r} must be integers")
        out.append(k)
    if not MIN_STATES <= len(out) <= MAX_STATES:
        raise ValueError(f"{who}: steps has {len(out)} states; the chain takes {MIN_STATES} to {MAX_STATES}")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{who}: steps={out!r} must ascend strictly")
    if 0 not in out:
        raise ValueError(f"{who}: steps={out!r} must hold 0, the neutral state")
    return tuple(out)


def _m_step(ns, ms, ss, qs, n_total, n_steps, ks, a, sigma, p, fit):
    """(a', sigma', p') of DESIGN.md 4.24, or None for a degenerate step.  ns, ms: the K sums of N_s and M_s over the
    cells; ks: the steps as floats."""
    states = range(len(ks))
    num = math.fsum(ks[s] * ms[s] for s in states)
    den = math.fsum((ks[s] * ks[s]) * ns[s] for s in states)
    if "amplitude" in fit and num > 0 and den > 0:
        a = num / den
    mu = [k * a for k in ks]
    if "sigma" in fit:
        var = ((qs - 2.0 * math.fsum(mu[s] * ms[s] for s in states))
               + math.fsum((mu[s] * mu[s]) * ns[s] for s in states)) / n_total
        if not (math.isfinite(var) and var > 0):
            return None
        sigma = math.sqrt(var)
    if "switch_prob" in fit and n_steps > 0:
        p = min(max(1.0 - ss / n_steps, _P_MIN), _P_MAX)
    try:
        ok = math.isfinite(a) and math.isfinite(1.0 / (2.0 * sigma * sigma))
    except ZeroDivisionError:
        ok = False
    return (a, sigma, p) if ok else None


def cnv_copy_states_fit(adata, use_rep="cnv", key_added="cnv_copy_states_fit", inplace=True, *, steps=None,
                        amplitude=None, sigma=None, switch_prob=None, fit=("amplitude", "sigma"), max_iter=25, tol=1e-4,
                        return_info=False):
    """Fit the parameters of the hidden Markov chain of :func:`infercnvpy_amd.tl.cnv_copy_states` to the matrix.

    Baum-Welch (expectation-maximisation) on the model of ``tl.cnv_copy_states`` with its levels on a lattice: K states
    with Gaussian emissions of means ``levels = [k * amplitude for k in steps]`` and one standard deviation ``sigma``,
    probability ``switch_prob`` of leaving a state between two windows, a uniform start, one chain per chromosome and
    cell.  Every iteration runs forward-backward on the GPU and updates the fitted parameters to the exact maximisers of
    the expected log-likelihood, which therefore never falls (but for rounding).  The result feeds the other functions
    through their keywords::

        cnv.tl.cnv_copy_states_fit(adata)
        cnv.tl.cnv_copy_states(adata, **adata.uns["cnv_copy_states_fit"]["params"])
        cnv.tl.cnv_copy_posteriors(adata)   # picks the parameters up from tl.cnv_copy_states

    The likelihood has more than one mode in ``amplitude``, and the fit ends in the one its start values lead to.  On the
    planted case of DESIGN.md 4.22 (24 cells, 130 windows, a step of 0.3, noise of 0.1) the default start, the
    difference-based ``sigma`` with a step of twice that, ends at a step of 0.297 to 0.299 in 4 to 5 iterations and
    leaves 15 to 25 wrong calls of 3 120, as the true parameters do.  From the start values of ``tl.cnv_copy_states``
    (the root mean square, 0.33, and twice that) the same fit ends at a step of 0.72 with all gains absorbed by the
    ``+1`` state (about 1 000 wrong calls), or at 0.44.  The levels stay on the lattice because an M-step with a free
    mean per state collapses two states onto each other or breaks their order.  ``amplitude=`` is the knob when you know
    the step better than the default start does.

    Requires running :func:`infercnvpy_amd.tl.infercnv` first.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, read as in ``tl.cnv_copy_states``.
        ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The result goes to ``adata.uns[key_added]``: ``params`` (``levels``, ``sigma``, ``switch_prob``: the keywords of
        ``tl.cnv_copy_states``), ``amplitude``, ``steps``, ``history`` (``amplitude``, ``sigma`` and ``switch_prob``
        before the first and after every iteration), ``n_iter``, ``converged`` and ``fit``.
    inplace
        If True, store the result in adata, otherwise return the params dict.
    steps
        The lattice: K integers, 2 <= K <= 8, strictly ascending, one of them 0 (the neutral state).  None:
        ``(-2, -1, 0, 1, 2, 3)``, the default levels of ``tl.cnv_copy_states``.
    amplitude, sigma, switch_prob
        Start values.  ``sigma=None``: the difference-based estimate of ``tl.cnv_changepoints``, ``sqrt(D / (2 M))`` over
        the adjacent windows of every chromosome, which does not count the level shifts themselves as noise; where it is
        0 or no chromosome has two windows, the root mean square of the matrix.  ``amplitude=None``: ``2 * sigma``.
        ``switch_prob=None``: ``1e-3``.  An all-zero matrix (``sigma == 0``) leaves ``sigma = 0`` and levels that are
        all 0.0, as ``tl.cnv_copy_states`` stores them, with ``n_iter = 0``.
    fit
        The parameters to fit: a non-empty subset of ``("amplitude", "sigma", "switch_prob")``; the others keep their
        start values.  The default leaves ``switch_prob`` alone, as ``tl.cnv_states_fit`` does and for its reason.
    max_iter
        The largest number of iterations, an int >= 1.
    tol
        The fit has converged when no fitted parameter moved by more than ``tol`` relative to its value before; finite
        and >= 0.
    return_info
        Also return a dict: ``history``, ``n_iter``, ``converged``, ``fit``, ``amplitude``, ``steps``, ``stopped``
        (``"degenerate"``, only when the fit ended so) and ``stage_ms`` (sums of squares and start values, all E-steps
        with their read-back; host clocks).

    Returns
    -------
    None when ``inplace`` or else the params dict, followed by the info dict when ``return_info``.  A step that would
    leave a variance that is not finite and > 0 (every stored value sits exactly on a level) ends the fit with the
    parameters of the iteration before, ``converged=False`` and a ``RuntimeWarning``.  Each iteration reads
    n x (2K + 1) float64 sums back; nothing of size n x W is allocated.  A non-finite value raises ``ValueError``, and so
    does a finite one whose emission overflows under the start values:
    ``(|x| + max(|levels[0]|, |levels[-1]|))^2 / (2 sigma^2)`` must be finite for the stored value of the largest
    magnitude.  The kernel keeps a cell's windows, K planes of forward variables and 2K + 1 sums per chromosome in LDS:
    ``8 (K + 1) W + 8 (2K + 1) n_chromosomes <= 163840`` bytes (2 883 windows for K = 6 and 23 chromosomes).
    """
    lattice = check_steps(DEFAULT_STEPS if steps is None else steps)
    k = len(lattice)
    ks = [float(s) for s in lattice]
    top = max(abs(ks[0]), abs(ks[-1]))
    p_start = 1e-3 if switch_prob is None else switch_prob
    key = f"X_{use_rep}"

    def options():
        # resolve() checked the keys, the shape and chr_pos: one start per chromosome
        w, n_chr = int(adata.obsm[key].shape[1]), len(adata.uns[use_rep]["chr_pos"])
        cap, lds = _lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, n_chr), _lib.ICV_COPY_POSTERIOR_LDS_BYTES
        if w > cap:
            raise ValueError(f"{_WHO}: {w} windows in {n_chr} chromosomes; the kernel keeps a cell's windows, the forward "
                             f"variables of K = {k} states and {2 * k + 1} sums per chromosome in {lds} bytes of LDS and "
                             f"takes at most {cap} windows")
        return _fit_options(fit, max_iter, tol, _WHO)

    def start_sigma(dm, bounds, rms):
        n, w = dm.shape
        d_host = _engine.changepoint_diffsq(dm, bounds).cpu().numpy()
        s = default_sigma(d_host.tolist(), n, w, int(bounds.shape[0]) - 1)
        return s if s > 0.0 else rms

    # the emission check of resolve() runs under the amplitude max(|levels[0]|, |levels[-1]|) once the step is known
    mo = resolve(adata, use_rep, _WHO, max_windows=_lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, 1),
                 keeps=f"a cell's windows, the forward variables of K = {k} states and {2 * k + 1} sums per chromosome "
                       f"({_lib.ICV_COPY_POSTERIOR_LDS_BYTES} bytes)", amplitude=amplitude, sigma=sigma,
                 switch_prob=p_start, log_switch=False, sum_of_squares=True, then=options, default_sigma=start_sigma,
                 n_states=k)
    fitted, tol_f = mo.rest
    n, bounds, dm, amp, sig, p, qs, t1 = mo.n, mo.bounds, mo.dm, mo.amp, mo.sig, mo.p, mo.qs, mo.t1
    z = lattice.index(0)
    if mo.h is not None:
        if not math.isfinite(top * amp):
            raise ValueError(f"{_WHO}: amplitude={amp!r} leaves float64's range at the step {int(top)}")
        check_emissions(_WHO, key, mo.x, mo.m, top * amp, mo.h, sig)
    n_total = float(n) * float(mo.w)

    cur = (amp, sig, p)
    history = [_as_dict(*cur)]
    n_iter, converged, stopped = 0, False, None
    if mo.h is not None:  # (an all-zero matrix has nothing to fit; later overflowing steps end as degenerate ones)
        n_steps = n * sum(max(int(b) - int(a) - 1, 0) for a, b in zip(bounds[:-1], bounds[1:]))
        for _ in range(max_iter):
            a_, s_, p_ = cur
            stats = _engine.copy_posterior_stats(dm, bounds, levels=[v * a_ for v in ks], neutral=z,
                                                 h=1.0 / (2.0 * s_ * s_), ps=1.0 - p_, pw=p_ / (k - 1))
            host = stats.cpu().numpy()  # one copy of n x (2K + 1)
            n_iter += 1
            sums = [math.fsum(host[:, j].tolist()) for j in range(2 * k + 1)]
            new = _m_step(sums[:k], sums[k:2 * k], sums[2 * k], qs, n_total, n_steps, ks, a_, s_, p_, fitted)
            if new is None:
                stopped = "degenerate"
                warnings.warn(f"{_WHO}: the update leaves no positive finite variance (every stored value sits on a "
                              f"level); the fit stops after {n_iter} iteration(s) with the parameters it had",
                              RuntimeWarning, stacklevel=2)
                break
            delta = max(abs(new[j] - cur[j]) / cur[j] for j in range(3) if _NAMES[j] in fitted)
            cur = new
            history.append(_as_dict(*cur))
            if delta <= tol_f:
                converged = True
                break
    t2 = time.perf_counter()
    params = {"levels": [v * cur[0] for v in ks], "sigma": cur[1], "switch_prob": cur[2]}
    info = None
    if return_info:
        info = {"history": history, "n_iter": n_iter, "converged": converged, "fit": fitted, "amplitude": cur[0],
                "steps": list(lattice), "stage_ms": {"rowsq": (t1 - mo.t0) * 1e3, "e_steps": (t2 - t1) * 1e3}}
        if stopped is not None:
            info["stopped"] = stopped
    if inplace:
        adata.uns[key_added] = {"params": params, "amplitude": cur[0], "steps": list(lattice), "history": history,
                                "n_iter": n_iter, "converged": converged, "fit": fitted}
        return (None, info) if return_info else None
    return (params, info) if return_info else params

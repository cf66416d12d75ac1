"""tl.cnv_states_fit: Baum-Welch fit of the parameters of ``tl.cnv_states`` (no counterpart in the reference).

``tl.cnv_states`` and its siblings run on a rule of thumb: ``sigma`` is the root mean square of the whole matrix, altered
windows included, so it overstates the noise, and ``amplitude = 2 * sigma`` then lands between noise and signal.  Here
expectation-maximisation fits ``amplitude``, ``sigma`` and, on request, ``switch_prob`` to the matrix.  The E-step is a
forward-backward pass along every chromosome of every cell on the GPU that leaves three sums per cell; the M-step is a
few scalar operations on the host.  Both follow the written contract of DESIGN.md 4.16 (float64, a fixed order), so the
fit is a pure function of (matrix, chr_pos, start values, fit, max_iter, tol) and equals ``tests/_fit_oracle.py`` bit for
bit.
"""
from __future__ import annotations

import math
import time
import warnings

from .. import _engine, _lib
from ._hmm import resolve

_NAMES = ("amplitude", "sigma", "switch_prob")
_P_MIN, _P_MAX = 1e-9, 0.5


def _m_step(gs, ds, ks, qs, n_total, n_steps, a, sigma, p, fit):
    """(a', sigma', p') of DESIGN.md 4.16, or None for a degenerate step."""
    if "amplitude" in fit and gs > 0 and ds > 0:
        a = ds / gs
    if "sigma" in fit:
        var = ((qs - (2.0 * a) * ds) + (a * a) * gs) / n_total
        if not (math.isfinite(var) and var > 0):
            return None
        sigma = math.sqrt(var)
    if "switch_prob" in fit and n_steps > 0:
        p = min(max(1.0 - ks / n_steps, _P_MIN), _P_MAX)
    try:
        ok = math.isfinite(a) and math.isfinite(1.0 / (2.0 * sigma * sigma))
    except ZeroDivisionError:
        ok = False
    return (a, sigma, p) if ok else None


def _fit_options(fit, max_iter, tol, who="tl.cnv_states_fit"):
    """(the fitted names in the order of _NAMES, tol as a float) of the checked ``fit``, ``max_iter`` and ``tol``."""
    if isinstance(fit, str):
        fit = (fit,)
    try:
        names = list(fit)
    except TypeError:
        raise ValueError(f"{who}: fit={fit!r} must be a sequence of parameter names") from None
    unknown = [k for k in names if k not in _NAMES]
    if unknown or not names:
        raise ValueError(f"{who}: fit={fit!r} must be a non-empty subset of {_NAMES}")
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 1:
        raise ValueError(f"{who}: max_iter={max_iter!r} must be an int >= 1")
    try:
        tol_f = float(tol)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: tol={tol!r} must be a number") from None
    if isinstance(tol, bool) or not (math.isfinite(tol_f) and tol_f >= 0.0):
        raise ValueError(f"{who}: tol={tol!r} must be finite and >= 0")
    return [k for k in _NAMES if k in names], tol_f


def _as_dict(a, sigma, p):
    return {"amplitude": a, "sigma": sigma, "switch_prob": p}


def cnv_states_fit(adata, use_rep="cnv", key_added="cnv_states_fit", inplace=True, *, amplitude=None, sigma=None,
                   switch_prob=None, fit=("amplitude", "sigma"), max_iter=25, tol=1e-4, return_info=False):
    """Fit the parameters of the hidden Markov chain of :func:`infercnvpy_amd.tl.cnv_states` to the matrix.

    Baum-Welch (expectation-maximisation) on the model of ``tl.cnv_states``: three states with Gaussian emissions of means
    ``(-amplitude, 0, +amplitude)`` and one standard deviation ``sigma``, probability ``switch_prob`` of leaving a state
    between two windows, a uniform start, one chain per chromosome and cell.  Every iteration runs forward-backward on
    the GPU and updates the fitted parameters to the exact maximisers of the expected log-likelihood, which therefore
    never falls (but for rounding).  The result feeds the other functions through their keywords::

        cnv.tl.cnv_states_fit(adata)
        cnv.tl.cnv_states(adata, **adata.uns["cnv_states_fit"]["params"])
        cnv.tl.cnv_posteriors(adata)   # picks the parameters up from tl.cnv_states

    Requires running :func:`infercnvpy_amd.tl.infercnv` first.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, read as in ``tl.cnv_states``.
        ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The result goes to ``adata.uns[key_added]``: ``params`` (``amplitude``, ``sigma``, ``switch_prob``), ``history``
        (the parameters before the first and after every iteration), ``n_iter``, ``converged`` and ``fit``.
    inplace
        If True, store the result in adata, otherwise return the params dict.
    amplitude, sigma, switch_prob
        Start values.  Each None resolves as in ``tl.cnv_states``: ``sigma`` to the root mean square of the matrix,
        ``amplitude`` to ``2 * sigma``, ``switch_prob`` to ``1e-3``.  An all-zero matrix (``sigma == 0``) leaves
        ``sigma = 0`` and ``amplitude = 0`` as ``tl.cnv_states`` stores them, with ``n_iter = 0``.
    fit
        The parameters to fit: a non-empty subset of ``("amplitude", "sigma", "switch_prob")``; the others keep their
        start values.  The default leaves ``switch_prob`` alone: it is a smoothing prior rather than a property of the
        data, and on the thresholded, zero-inflated ``X_cnv`` a fitted value mostly measures isolated blips.
    max_iter
        The largest number of iterations, an int >= 1.
    tol
        The fit has converged when no fitted parameter moved by more than ``tol`` relative to its value before; finite
        and >= 0.
    return_info
        Also return a dict: ``history``, ``n_iter``, ``converged``, ``fit``, ``stopped`` (``"degenerate"``, only when
        the fit ended so) and ``stage_ms`` (sums of squares, all E-steps with their read-back; host clocks).

    Returns
    -------
    None when ``inplace`` or else the params dict, followed by the info dict when ``return_info``.  A step that would
    leave a variance that is not finite and > 0 (every stored value sits exactly on a mean) ends the fit with the
    parameters of the iteration before, ``converged=False`` and a ``RuntimeWarning``.  Each iteration reads n x 3 float64
    sums back; nothing of size n x W is allocated.  A non-finite value raises ``ValueError``, and so does a finite one
    whose emission overflows under the start values: ``(|x| + amplitude)^2 / (2 sigma^2)`` must be finite for the stored
    value of the largest magnitude.
    """
    mo = resolve(adata, use_rep, "tl.cnv_states_fit", max_windows=_lib.ICV_POSTERIOR_MAX_WINDOWS,
                 keeps="a cell's windows and forward variables", amplitude=amplitude, sigma=sigma,
                 switch_prob=1e-3 if switch_prob is None else switch_prob, log_switch=False, sum_of_squares=True,
                 then=lambda: _fit_options(fit, max_iter, tol))
    fitted, tol_f = mo.rest
    n, bounds, dm, amp, sig, p, qs, t1 = mo.n, mo.bounds, mo.dm, mo.amp, mo.sig, mo.p, mo.qs, mo.t1
    n_total = float(n) * float(mo.w)

    cur = (amp, sig, p)
    history = [_as_dict(*cur)]
    n_iter, converged, stopped = 0, False, None
    if mo.h is not None:  # (an all-zero matrix has nothing to fit; later overflowing steps end as degenerate ones)
        n_steps = n * sum(max(int(b) - int(a) - 1, 0) for a, b in zip(bounds[:-1], bounds[1:]))
        for _ in range(max_iter):
            a_, s_, p_ = cur
            stats = _engine.posterior_stats(dm, bounds, amplitude=a_, h=1.0 / (2.0 * s_ * s_), ps=1.0 - p_, pw=p_ / 2.0)
            host = stats.cpu().numpy()  # one copy of n x 3
            n_iter += 1
            gs, ds, ks = (math.fsum(host[:, k].tolist()) for k in range(3))
            new = _m_step(gs, ds, ks, qs, n_total, n_steps, a_, s_, p_, fitted)
            if new is None:
                stopped = "degenerate"
                warnings.warn("tl.cnv_states_fit: the update leaves no positive finite variance (every stored value "
                              f"sits on a state's mean); the fit stops after {n_iter} iteration(s) with the parameters "
                              "it had", RuntimeWarning, stacklevel=2)
                break
            delta = max(abs(new[k] - cur[k]) / cur[k] for k in range(3) if _NAMES[k] in fitted)
            cur = new
            history.append(_as_dict(*cur))
            if delta <= tol_f:
                converged = True
                break
    t2 = time.perf_counter()
    params = _as_dict(*cur)
    info = None
    if return_info:
        info = {"history": history, "n_iter": n_iter, "converged": converged, "fit": fitted,
                "stage_ms": {"rowsq": (t1 - mo.t0) * 1e3, "e_steps": (t2 - t1) * 1e3}}
        if stopped is not None:
            info["stopped"] = stopped
    if inplace:
        adata.uns[key_added] = {"params": params, "history": history, "n_iter": n_iter, "converged": converged,
                                "fit": fitted}
        return (None, info) if return_info else None
    return (params, info) if return_info else params

"""tl.cnv_copy_posteriors and tl.cnv_copy_states_filter: the confidence of the calls of ``tl.cnv_copy_states`` (no
counterpart in the reference).

In R inferCNV the Bayesian step belongs to the multi-level model: every called region gets a posterior, and a region whose
mean P(normal) exceeds ``BayesMaxPNormal`` is dropped.  Here forward-backward runs along every chromosome of every cell on
the GPU, on the K-state model of ``tl.cnv_copy_states``, by the written contract of DESIGN.md 4.23 (the K-state form of
4.15: float64, a fixed order, the written exponential of ``tl.tsne``), and the filter forms the mean P(neutral) of every
run of one level from integer sums.  Both equal ``tests/_copy_posterior_oracle.py`` bit for bit; with
``levels=(-a, 0.0, a)`` the posteriors are the bytes of ``tl.cnv_posteriors``.
"""
from __future__ import annotations

import sys
import time

from .. import _engine, _lib
from ._copy_states import DEFAULT_STEPS, check_levels
from ._hmm import call_matrix, check_emissions, chromosome_bounds, resolve

_WHO = "tl.cnv_copy_posteriors"


def plane_names(k, z):
    """The names of the K planes in state order, by the state's distance from the neutral one:
    ``loss2, loss1, neutral, gain1, ...``."""
    return [f"loss{z - s}" if s < z else "neutral" if s == z else f"gain{s - z}" for s in range(k)]


def cnv_copy_posteriors(adata, use_rep="cnv", key_added="cnv_copy_posterior", inplace=True, *, levels=None,
                        amplitude=None, sigma=None, switch_prob=None, states_key="cnv_copy_states", all_states=False,
                        return_info=False):
    """Posterior probability of every window of every cell being neutral (and, on request, at every other level).

    Forward-backward on the hidden Markov chain of :func:`infercnvpy_amd.tl.cnv_copy_states`: K states with Gaussian
    emissions of means ``levels`` and standard deviation ``sigma``, probability ``switch_prob`` of leaving a state between
    two windows (each of the other K - 1 states gets an equal share), one chain per chromosome and cell.  Requires running
    :func:`infercnvpy_amd.tl.infercnv` first.  :func:`infercnvpy_amd.tl.cnv_copy_states_fit` fits the model to the matrix;
    called with its ``params``, ``tl.cnv_copy_states`` leaves them where this function picks them up.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, read as in ``tl.cnv_copy_states``.
        ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        P(neutral) goes to ``adata.obsm[f"X_{key_added}_neutral"]`` (float64 n x W); with ``all_states`` one plane per
        state, named by its distance from neutral: ``..._loss2``, ``..._loss1``, ``..._neutral``, ``..._gain1``, ...;
        ``{"params": {"levels", "neutral", "sigma", "switch_prob"}, "planes": [the names in state order]}`` to
        ``adata.uns[key_added]``.
    inplace
        If True, store the result in adata, otherwise return it.
    levels, amplitude, sigma, switch_prob
        The model.  If all four are None and ``adata.uns[states_key]["params"]`` exists, it is taken from there: the
        posteriors then belong to the calls ``tl.cnv_copy_states`` made.  Otherwise each None resolves as in
        ``tl.cnv_copy_states`` (``levels`` to six steps of ``amplitude``, that to ``2 * sigma``, ``sigma`` to the root
        mean square of the matrix) and ``switch_prob`` to ``1e-3``.  An all-zero matrix (``sigma == 0``) gives
        P(neutral) = 1.
    states_key
        Where ``tl.cnv_copy_states`` left its parameters.
    all_states
        Also return / store the planes of the other states.
    return_info
        Also return a dict: ``levels``, ``neutral``, ``sigma``, ``switch_prob``, ``n_chromosomes`` and ``stage_ms`` (sums
        of squares, chains; host clocks, the second one waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``neutral`` or, with ``all_states``, the tuple of the K planes
    in state order, followed by the info dict when ``return_info``.  Host input gives host numpy arrays; device input
    (``PackedCsr``, CUDA tensor) leaves CUDA float64 tensors and nothing is read back after the non-finite flag.  A
    non-finite value raises ``ValueError``, and so does a finite one whose emission overflows:
    ``(|x| + max(|levels[0]|, |levels[-1]|))^2 / (2 sigma^2)`` must be finite for the stored value of the largest
    magnitude.  The kernel keeps a cell's windows and K planes of forward variables in LDS: at most
    ``ICV_COPY_POSTERIOR_MAX_WINDOWS(K) = 163840 // (8 (K + 1))`` windows (3 413 for K = 6).
    """
    if levels is not None and amplitude is not None:
        raise ValueError(f"{_WHO}: levels and amplitude are both given; amplitude only spaces the default levels")
    mu = z = None
    zero_model = False
    if levels is None and amplitude is None and sigma is None and switch_prob is None and states_key in adata.uns:
        stored = adata.uns[states_key]
        if isinstance(stored, dict) and "params" in stored:
            par = stored["params"]
            levels, sigma, switch_prob = par["levels"], par["sigma"], par["switch_prob"]
            zero_model = sigma == 0  # (what tl.cnv_copy_states leaves for an all-zero matrix: its levels are all 0)
            if zero_model:
                mu, z = [float(v) for v in levels], int(par["neutral"])
    if levels is not None and not zero_model:
        mu, z = check_levels(levels, _WHO)
    k = len(DEFAULT_STEPS) if mu is None else len(mu)
    if switch_prob is None:
        switch_prob = 1e-3

    def other_states_share():
        # rule 1 divides switch_prob by K - 1, resolve() tried it with 2
        if not float(switch_prob) / (k - 1) >= sys.float_info.min:
            raise ValueError(f"{_WHO}: switch_prob={switch_prob!r} is too close to 0 or 1 for float64")

    cap = _lib.ICV_COPY_POSTERIOR_MAX_WINDOWS(k)
    # rule 7 with given levels is resolve()'s own check under the amplitude max(|levels[0]|, |levels[-1]|)
    mo = resolve(adata, use_rep, _WHO, max_windows=cap,
                 keeps=f"a cell's windows and the forward variables of K = {k} states",
                 amplitude=amplitude if mu is None else max(abs(mu[0]), abs(mu[-1])), sigma=sigma,
                 switch_prob=switch_prob, log_switch=False, sum_of_squares=False, zero_model=zero_model,
                 then=other_states_share)
    n, w, bounds, sig, p, on_device = mo.n, mo.w, mo.bounds, mo.sig, mo.p, mo.on_device
    if mu is None:
        mu = [float(s) * mo.amp for s in DEFAULT_STEPS]
        z = DEFAULT_STEPS.index(0)
        if mo.h is not None:
            mu, z = check_levels(mu, _WHO)
            check_emissions(_WHO, f"X_{use_rep}", mo.x, mo.m, max(abs(mu[0]), abs(mu[-1])), mo.h, sig)
    names = plane_names(k, z)
    torch = _engine._torch()
    with torch.cuda.device(mo.dm.device):
        if mo.h is None:  # an all-zero matrix: every window is neutral
            neutral = torch.ones((n, w), dtype=torch.float64, device="cuda")
            planes = torch.zeros((k, n, w), dtype=torch.float64, device="cuda") if all_states else None
        else:
            neutral, planes = _engine.copy_posterior_chains(mo.dm, bounds, levels=mu, neutral=z, h=mo.h, ps=1.0 - p,
                                                            pw=p / (k - 1), all_states=all_states)
        info = None
        if return_info:
            torch.cuda.current_stream().synchronize()
            info = {"levels": list(mu), "neutral": z, "sigma": sig, "switch_prob": p,
                    "n_chromosomes": int(bounds.shape[0]) - 1,
                    "stage_ms": {"rowsq": (mo.t1 - mo.t0) * 1e3, "chains": (time.perf_counter() - mo.t1) * 1e3}}
        if not on_device:
            neutral = neutral.cpu().numpy()
            if all_states:
                planes = planes.cpu().numpy()
    result = tuple(neutral if s == z else planes[s] for s in range(k)) if all_states else neutral
    if inplace:
        if all_states:
            for name, plane in zip(names, result):
                adata.obsm[f"X_{key_added}_{name}"] = plane
        else:
            adata.obsm[f"X_{key_added}_neutral"] = neutral
        adata.uns[key_added] = {"params": {"levels": list(mu), "neutral": z, "sigma": sig, "switch_prob": p},
                                "planes": names if all_states else ["neutral"]}
        return (result, info) if return_info else None
    return (result, info) if return_info else result


def cnv_copy_states_filter(adata, use_rep="cnv_copy_states", posterior_key="cnv_copy_posterior", cnv_key="cnv",
                           key_added="cnv_copy_states_filtered", max_p_normal=0.5, inplace=True, return_info=False):
    """Reset to neutral every called run of one level whose mean P(neutral) is above ``max_p_normal`` (R inferCNV's
    ``BayesMaxPNormal``).

    A run is a maximal stretch of one level other than 0 inside one chromosome: ``+1 +1 +2 +2`` is two runs, each with
    its own verdict.  Requires :func:`infercnvpy_amd.tl.cnv_copy_states` and
    :func:`infercnvpy_amd.tl.cnv_copy_posteriors`.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` holds the int8 levels (n x W, in [-7, 7]), a host array or a CUDA tensor.
    posterior_key
        ``adata.obsm[f"X_{posterior_key}_neutral"]`` holds P(neutral) (float64 n x W), a host array or a CUDA tensor.
    cnv_key
        ``adata.uns[cnv_key]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The filtered levels go to ``adata.obsm[f"X_{key_added}"]`` (int8), the same clipped to -1 / 0 / +1 to
        ``adata.obsm[f"X_{key_added}_sign"]`` (``tl.cnv_segments(adata, groupby, use_rep=key_added + "_sign")`` takes it
        as it is), the share of each cell's windows that are still not neutral to ``adata.obs[key_added + "_fraction"]``
        (float64), the number of runs removed per cell to ``adata.obs[key_added + "_removed"]`` (int32),
        ``{"params": {"max_p_normal", "use_rep", "posterior_key"}, "chr_pos": a copy}`` to ``adata.uns[key_added]``.
    max_p_normal
        A finite number in [0, 1].  With ``q = rint(P 2^40)`` per window, a run of L windows is reset iff
        ``sum(q) / (L 2^40) > max_p_normal``: integer sums, so the verdict does not depend on the order of summation.
    inplace
        If True, store the result in adata, otherwise return ``(filtered, sign, fraction, removed)``.
    return_info
        Also return a dict: ``n_removed`` and ``stage_ms`` (host clock, waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(filtered, sign, fraction, removed)``, followed by the info
    dict when ``return_info``.  When levels and posteriors are both host arrays the results are host arrays; otherwise
    they are CUDA tensors (``inplace=True`` copies the two per-cell vectors back for ``adata.obs``).  A posterior that is
    not a number in [0, 1] or a level outside [-7, 7] raises ``ValueError`` (one flag read back from the device).
    """
    who = "tl.cnv_copy_states_filter"
    key, pkey = f"X_{use_rep}", f"X_{posterior_key}_neutral"
    x, post, n, w = call_matrix(adata, who, key, cnv_key, "`tl.infercnv`?", pkey)
    if w > _lib.ICV_FILTER_MAX_WINDOWS:
        raise ValueError(f"{who}: {w} windows; a run's int64 sum takes at most {_lib.ICV_FILTER_MAX_WINDOWS}")
    bounds = chromosome_bounds(adata.uns[cnv_key]["chr_pos"], w)
    try:
        thr = float(max_p_normal)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: max_p_normal={max_p_normal!r} must be a number in [0, 1]") from None
    if isinstance(max_p_normal, bool) or not 0.0 <= thr <= 1.0:
        raise ValueError(f"{who}: max_p_normal={max_p_normal!r} must lie in [0, 1]")

    torch = _engine._torch()
    on_device = isinstance(x, torch.Tensor) or isinstance(post, torch.Tensor)
    t0 = time.perf_counter()
    states = _engine.dense_input(x)
    with torch.cuda.device(states.device):
        p_dev = _engine.dense_input(post).to(states.device)
        filtered, sign, count, removed, bad = _engine.copy_states_filter(states, p_dev, bounds, thr)
        fraction = _engine.states_fraction(count, w)
        if int(bad.item()):
            raise ValueError(f"{who}: {pkey} has values that are not numbers in [0, 1], or {key} has levels outside "
                             "[-7, 7]")
        info = None
        if return_info:
            info = {"n_removed": int(removed.sum().item()), "stage_ms": {"filter": (time.perf_counter() - t0) * 1e3}}
        if not on_device:
            filtered, sign = filtered.cpu().numpy(), sign.cpu().numpy()
            fraction, removed = fraction.cpu().numpy(), removed.cpu().numpy()
    if inplace:
        adata.obsm[f"X_{key_added}"] = filtered
        adata.obsm[f"X_{key_added}_sign"] = sign
        adata.obs[key_added + "_fraction"] = fraction.cpu().numpy() if on_device else fraction
        adata.obs[key_added + "_removed"] = removed.cpu().numpy() if on_device else removed
        adata.uns[key_added] = {"params": {"max_p_normal": thr, "use_rep": use_rep, "posterior_key": posterior_key},
                                "chr_pos": dict(adata.uns[cnv_key]["chr_pos"])}
        return (filtered, sign, fraction, removed, info) if return_info else None
    return (filtered, sign, fraction, removed, info) if return_info else (filtered, sign, fraction, removed)

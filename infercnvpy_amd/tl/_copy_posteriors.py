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

import time

from .. import _engine, _lib
from ._hmm import resolve_levels
from ._posteriors import _filter_runs

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
    zero_levels = None
    if levels is None and amplitude is None and sigma is None and switch_prob is None and states_key in adata.uns:
        stored = adata.uns[states_key]
        if isinstance(stored, dict) and "params" in stored:
            par = stored["params"]
            levels, sigma, switch_prob = par["levels"], par["sigma"], par["switch_prob"]
            if sigma == 0:  # (what tl.cnv_copy_states leaves for an all-zero matrix: its levels are all 0)
                zero_levels = [float(v) for v in levels], int(par["neutral"])
    mo, mu, z, k = resolve_levels(
        adata, use_rep, _WHO, levels=levels, amplitude=amplitude, sigma=sigma,
        switch_prob=1e-3 if switch_prob is None else switch_prob, log_switch=False, zero_levels=zero_levels,
        max_windows=_lib.ICV_COPY_POSTERIOR_MAX_WINDOWS,
        keeps=lambda k: f"a cell's windows and the forward variables of K = {k} states")
    n, w, bounds, sig, p, on_device = mo.n, mo.w, mo.bounds, mo.sig, mo.p, mo.on_device
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
    return _filter_runs(adata, "tl.cnv_copy_states_filter", _engine.copy_states_filter, "levels outside [-7, 7]", True,
                        use_rep, posterior_key, cnv_key, key_added, max_p_normal, inplace, return_info)

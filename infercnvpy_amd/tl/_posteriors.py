"""tl.cnv_posteriors and tl.cnv_states_filter: the confidence of the calls of ``tl.cnv_states`` (no counterpart in the
reference).

R inferCNV's HMM pipeline ends in posterior probabilities: every called segment whose mean P(normal) exceeds
``BayesMaxPNormal`` is dropped.  Here forward-backward runs along every chromosome of every cell on the GPU, on the
three-state model of ``tl.cnv_states``, by the written contract of DESIGN.md 4.15 (float64, a fixed order, the written
exponential of ``tl.tsne``), and the filter forms every run's mean P(neutral) from integer sums.  Both equal
``tests/_posterior_oracle.py`` bit for bit.
"""
from __future__ import annotations

import time

from .. import _engine, _lib
from ._hmm import call_matrix, chromosome_bounds, resolve


def cnv_posteriors(adata, use_rep="cnv", key_added="cnv_posterior", inplace=True, *, amplitude=None, sigma=None,
                   switch_prob=None, states_key="cnv_states", all_states=False, return_info=False):
    """Posterior probability of every window of every cell being neutral (and, on request, lost or gained).

    Forward-backward on the hidden Markov chain of :func:`infercnvpy_amd.tl.cnv_states`: three states with Gaussian
    emissions of means ``(-amplitude, 0, +amplitude)`` and standard deviation ``sigma``, probability ``switch_prob`` of
    leaving a state between two windows, one chain per chromosome and cell.  Requires running
    :func:`infercnvpy_amd.tl.infercnv` first.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W): a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor, read as in ``tl.cnv_states``.
        ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        P(neutral) goes to ``adata.obsm[f"X_{key_added}_neutral"]`` (float64 n x W), with ``all_states`` P(loss) and
        P(gain) to ``..._loss`` and ``..._gain``; the resolved parameters to ``adata.uns[key_added]["params"]``.
    inplace
        If True, store the result in adata, otherwise return it.
    amplitude, sigma, switch_prob
        The model.  If all three are None and ``adata.uns[states_key]["params"]`` exists, they are taken from there:
        the posteriors then belong to the calls ``tl.cnv_states`` made.  Otherwise each None resolves as in
        ``tl.cnv_states``: ``sigma`` to the root mean square of the matrix, ``amplitude`` to ``2 * sigma``,
        ``switch_prob`` to ``1e-3``.  An all-zero matrix (``sigma == 0``) gives P(neutral) = 1.
    states_key
        Where ``tl.cnv_states`` left its parameters.
    all_states
        Also return / store P(loss) and P(gain).
    return_info
        Also return a dict: ``amplitude``, ``sigma``, ``switch_prob``, ``n_chromosomes`` and ``stage_ms`` (sums of
        squares, chains; host clocks, the second one waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``neutral`` or, with ``all_states``,
    ``(loss, neutral, gain)``, followed by the info dict when ``return_info``.  Host input gives host numpy arrays;
    device input (``PackedCsr``, CUDA tensor) leaves CUDA float64 tensors and nothing is read back after the
    non-finite flag.  A non-finite value raises ``ValueError``, and so does a finite one whose emission overflows:
    ``(|x| + amplitude)^2 / (2 sigma^2)`` must be finite for the stored value of the largest magnitude (read back with
    the flag); the posteriors of its chromosome would be 0 / 0 otherwise.
    """
    from_states = False
    if amplitude is None and sigma is None and switch_prob is None and states_key in adata.uns:
        stored = adata.uns[states_key]
        if isinstance(stored, dict) and "params" in stored:
            amplitude, sigma, switch_prob = (stored["params"][k] for k in ("amplitude", "sigma", "switch_prob"))
            from_states = True
    mo = resolve(adata, use_rep, "tl.cnv_posteriors", max_windows=_lib.ICV_POSTERIOR_MAX_WINDOWS,
                 keeps="a cell's windows and forward variables", amplitude=amplitude, sigma=sigma,
                 switch_prob=1e-3 if switch_prob is None else switch_prob, log_switch=False, sum_of_squares=False,
                 zero_model=from_states and sigma == 0)  # (what tl.cnv_states leaves for an all-zero matrix)
    n, w, bounds, amp, sig, p, on_device = mo.n, mo.w, mo.bounds, mo.amp, mo.sig, mo.p, mo.on_device
    torch = _engine._torch()
    with torch.cuda.device(mo.dm.device):
        if mo.h is None:  # an all-zero matrix: every window is neutral
            neutral = torch.ones((n, w), dtype=torch.float64, device="cuda")
            loss = torch.zeros((n, w), dtype=torch.float64, device="cuda") if all_states else None
            gain = torch.zeros((n, w), dtype=torch.float64, device="cuda") if all_states else None
        else:
            neutral, loss, gain = _engine.posterior_chains(mo.dm, bounds, amplitude=amp, h=mo.h, ps=1.0 - p, pw=p / 2.0,
                                                           all_states=all_states)
        info = None
        if return_info:
            torch.cuda.current_stream().synchronize()
            info = {"amplitude": amp, "sigma": sig, "switch_prob": p, "n_chromosomes": int(bounds.shape[0]) - 1,
                    "stage_ms": {"rowsq": (mo.t1 - mo.t0) * 1e3, "chains": (time.perf_counter() - mo.t1) * 1e3}}
        if not on_device:
            neutral = neutral.cpu().numpy()
            if all_states:
                loss, gain = loss.cpu().numpy(), gain.cpu().numpy()
    result = (loss, neutral, gain) if all_states else neutral
    if inplace:
        adata.obsm[f"X_{key_added}_neutral"] = neutral
        if all_states:
            adata.obsm[f"X_{key_added}_loss"] = loss
            adata.obsm[f"X_{key_added}_gain"] = gain
        adata.uns[key_added] = {"params": {"amplitude": amp, "sigma": sig, "switch_prob": p}}
        return (result, info) if return_info else None
    return (result, info) if return_info else result


def cnv_states_filter(adata, use_rep="cnv_states", posterior_key="cnv_posterior", cnv_key="cnv",
                      key_added="cnv_states_filtered", max_p_normal=0.5, inplace=True, return_info=False):
    """Reset to neutral every called segment whose mean P(neutral) is above ``max_p_normal`` (R inferCNV's
    ``BayesMaxPNormal``).

    A segment is a maximal run of -1 or of +1 inside one chromosome, as :func:`infercnvpy_amd.tl.cnv_segments` defines
    it.  Requires :func:`infercnvpy_amd.tl.cnv_states` and :func:`infercnvpy_amd.tl.cnv_posteriors`.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` holds the int8 calls (n x W), a host array or a CUDA tensor.
    posterior_key
        ``adata.obsm[f"X_{posterior_key}_neutral"]`` holds P(neutral) (float64 n x W), a host array or a CUDA tensor.
    cnv_key
        ``adata.uns[cnv_key]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The filtered calls go to ``adata.obsm[f"X_{key_added}"]`` (int8; ``tl.cnv_segments(..., use_rep=key_added)``
        reads them), the share of each cell's windows that are still not neutral to
        ``adata.obs[key_added + "_fraction"]`` (float64), the number of segments removed per cell to
        ``adata.obs[key_added + "_removed"]`` (int32), the parameters to ``adata.uns[key_added]["params"]``.
    max_p_normal
        A finite number in [0, 1].  With ``q = rint(P 2^40)`` per window, a run of L windows is reset iff
        ``sum(q) / (L 2^40) > max_p_normal``: integer sums, so the verdict does not depend on the order of summation.
    inplace
        If True, store the result in adata, otherwise return ``(filtered, fraction, removed)``.
    return_info
        Also return a dict: ``n_removed`` and ``stage_ms`` (host clock, waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(filtered, fraction, removed)``, followed by the info dict
    when ``return_info``.  When calls and posteriors are both host arrays the results are host arrays; otherwise they
    are CUDA tensors (``inplace=True`` copies the two per-cell vectors back for ``adata.obs``).  A posterior that is
    not a number in [0, 1] or a call other than -1 / 0 / +1 raises ``ValueError`` (one flag read back from the device).
    """
    return _filter_runs(adata, "tl.cnv_states_filter", _engine.states_filter, "values other than -1, 0 and +1", False,
                        use_rep, posterior_key, cnv_key, key_added, max_p_normal, inplace, return_info)


def _filter_runs(adata, who, engine_call, bad_calls, with_sign, use_rep, posterior_key, cnv_key, key_added, max_p_normal,
                 inplace, return_info):
    """The body of ``tl.cnv_states_filter`` and ``tl.cnv_copy_states_filter``.  ``engine_call``: ``_engine.states_filter``
    or ``_engine.copy_states_filter``; ``bad_calls``: what the calls hold when the kernel refuses them, for the message;
    ``with_sign``: there is a second plane, the filtered calls clipped to -1 / 0 / +1, stored with a copy of ``chr_pos``
    so that ``tl.cnv_segments`` takes it as it is."""
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
        *planes, count, removed, bad = engine_call(states, p_dev, bounds, thr)
        fraction = _engine.states_fraction(count, w)
        if int(bad.item()):
            raise ValueError(f"{who}: {pkey} has values that are not numbers in [0, 1], or {key} has {bad_calls}")
        info = None
        if return_info:
            info = {"n_removed": int(removed.sum().item()), "stage_ms": {"filter": (time.perf_counter() - t0) * 1e3}}
        if not on_device:
            planes = [t.cpu().numpy() for t in planes]
            fraction, removed = fraction.cpu().numpy(), removed.cpu().numpy()
    result = (*planes, fraction, removed)  # (filtered, [sign,] fraction, removed)
    if inplace:
        adata.obsm[f"X_{key_added}"] = planes[0]
        if with_sign:
            adata.obsm[f"X_{key_added}_sign"] = planes[1]
        adata.obs[key_added + "_fraction"] = fraction.cpu().numpy() if on_device else fraction
        adata.obs[key_added + "_removed"] = removed.cpu().numpy() if on_device else removed
        adata.uns[key_added] = {"params": {"max_p_normal": thr, "use_rep": use_rep, "posterior_key": posterior_key}}
        if with_sign:
            adata.uns[key_added]["chr_pos"] = dict(adata.uns[cnv_key]["chr_pos"])
        return (*result, info) if return_info else None
    return (*result, info) if return_info else result

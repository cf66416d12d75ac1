"""tl.cnv_copy_states: per-cell multi-level copy-number calls of ``X_cnv`` (no counterpart in the reference).

``tl.cnv_states`` knows one amplitude: a one-copy gain and a two-copy gain both come out as ``+1``.  R inferCNV's default
model has six states (complete loss, one-copy loss, neutral, one-, two- and a higher gain); here a K-state Viterbi chain,
2 <= K <= 8, with Gaussian emissions of a common ``sigma`` and the state means ``levels`` runs along every chromosome of
every cell on the GPU by the written contract of DESIGN.md 4.22: float64 adds, multiplies and compares in a fixed order,
so the calls are a pure function of (matrix, chr_pos, levels, sigma, switch_prob) and equal
``tests/_copy_states_oracle.py`` bit for bit.  With ``levels=(-a, 0.0, a)`` the rules are those of ``tl.cnv_states`` and
so are the bytes.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine, _lib
from ._hmm import DEFAULT_STEPS, MAX_STATES, MIN_STATES, check_levels, resolve_levels  # noqa: F401 (re-exported)

_WHO = "tl.cnv_copy_states"


def cnv_copy_states(adata, use_rep="cnv", key_added="cnv_copy_states", inplace=True, *, levels=None, amplitude=None,
                    sigma=None, switch_prob=1e-3, return_info=False):
    """Call the copy-number level of every window of every cell: 0 neutral, -1 / +1 one step down / up, -2 / +2 two ...

    A K-state hidden Markov chain with Gaussian emissions of means ``levels`` and standard deviation ``sigma`` runs along
    each chromosome of each cell; the most likely path (Viterbi) is the call, reported as the state's distance from the
    neutral one.  Chains never cross a chromosome boundary.  Requires running :func:`infercnvpy_amd.tl.infercnv` first.
    :func:`infercnvpy_amd.tl.cnv_copy_states_fit` fits ``levels`` and ``sigma`` to the matrix in place of the defaults.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) is called: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor.  Stored values are used as float64, an entry that is
        not stored is 0.0.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The calls go to ``adata.obsm[f"X_{key_added}"]`` (int8, in ``[-z, K - 1 - z]`` with z the index of the neutral
        level), the calls clipped to -1 / 0 / +1 to ``adata.obsm[f"X_{key_added}_sign"]`` (the format of
        :func:`cnv_states`: ``tl.cnv_segments(adata, use_rep=key_added + "_sign")`` takes it as it is), the share of each
        cell's windows that are not neutral to ``adata.obs[key_added + "_fraction"]`` (float64: an integer count divided
        by W), ``{"params": {"levels", "neutral", "sigma", "switch_prob"}, "chr_pos": a copy}`` to
        ``adata.uns[key_added]``.
    inplace
        If True, store the result in adata, otherwise return ``(states, sign, fraction)``.
    levels
        The K state means, 2 <= K <= 8: finite, strictly ascending, exactly one of them 0.0 (the neutral state).  None:
        ``[k * amplitude for k in (-2, -1, 0, 1, 2, 3)]``, the six states of R inferCNV's default model.  Not together
        with ``amplitude``.
    amplitude
        The step between the default levels; None: ``2 * sigma``.
    sigma
        Standard deviation of the emissions; None: the root mean square of the matrix over all n W windows, as in
        :func:`cnv_states`.  An all-zero matrix (``sigma == 0``) gives all-neutral calls.
    switch_prob
        Probability of leaving a state between two windows, in (0, 1); each of the other K - 1 states gets an equal share.
    return_info
        Also return a dict: ``levels``, ``neutral``, ``sigma``, ``n_chromosomes`` and ``stage_ms`` (sums of squares,
        chains; host clocks, the second one waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(states, sign, fraction)``, followed by the info dict when
    ``return_info``.  Host input gives host numpy arrays.  Device input (``PackedCsr``, CUDA tensor) leaves ``states`` and
    ``sign`` on the device as CUDA int8 tensors; with ``inplace=False`` the fraction is a CUDA float64 tensor as well and
    the call returns without waiting for the chains, while ``inplace=True`` copies the n counts back for ``adata.obs``.
    A non-finite value raises ``ValueError``, and so does a finite one so large that its emission overflows:
    ``(|x| + max(|levels[0]|, |levels[-1]|))^2 / (2 sigma^2)`` must be finite for the stored value of the largest
    magnitude.
    """
    mo, mu, z, k = resolve_levels(adata, use_rep, _WHO, levels=levels, amplitude=amplitude, sigma=sigma,
                                  switch_prob=switch_prob, log_switch=True,
                                  max_windows=lambda k: _lib.ICV_COPY_STATES_MAX_WINDOWS, keeps=lambda k: "a cell's windows")
    n, w, bounds, sig, p, on_device = mo.n, mo.w, mo.bounds, mo.sig, mo.p, mo.on_device
    torch = _engine._torch()
    with torch.cuda.device(mo.dm.device):
        if mo.h is None:  # an all-zero matrix: nothing to call
            states = torch.zeros((n, w), dtype=torch.int8, device="cuda")
            sign = torch.zeros((n, w), dtype=torch.int8, device="cuda")
            count = torch.zeros(n, dtype=torch.int32, device="cuda")
        else:
            states, sign, count = _engine.copy_states_viterbi(mo.dm, bounds, levels=mu, neutral=z, h=mo.h,
                                                              stay=math.log(1.0 - p), sw=math.log(p / (k - 1)))
        info = None
        if return_info:
            torch.cuda.current_stream().synchronize()
            info = {"levels": list(mu), "neutral": z, "sigma": sig, "n_chromosomes": int(bounds.shape[0]) - 1,
                    "stage_ms": {"rowsq": (mo.t1 - mo.t0) * 1e3, "viterbi": (time.perf_counter() - mo.t1) * 1e3}}
        if on_device and not inplace:
            fraction = _engine.states_fraction(count, w)
        else:
            fraction = count.cpu().numpy().astype(np.float64) / float(w)
        if not on_device:
            states, sign = states.cpu().numpy(), sign.cpu().numpy()
    if inplace:
        adata.obsm[f"X_{key_added}"] = states
        adata.obsm[f"X_{key_added}_sign"] = sign
        adata.obs[key_added + "_fraction"] = fraction
        adata.uns[key_added] = {"params": {"levels": list(mu), "neutral": z, "sigma": sig, "switch_prob": p},
                                "chr_pos": dict(adata.uns[use_rep]["chr_pos"])}
        return (states, sign, fraction, info) if return_info else None
    return (states, sign, fraction, info) if return_info else (states, sign, fraction)

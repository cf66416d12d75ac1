"""tl.cnv_states: per-cell loss / neutral / gain calls of ``X_cnv`` (no counterpart in the reference).

R inferCNV answers "which windows of which cells are gained or lost" with an HMM along the genome; the reference never
did.  Here a three-state Viterbi chain runs along every chromosome of every cell on the GPU by the written contract of
DESIGN.md 4.13: float64 adds, multiplies and compares in a fixed order, so the calls are a pure function of
(matrix, chr_pos, amplitude, sigma, switch_prob) and equal ``tests/_states_oracle.py`` bit for bit.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .. import _engine, _lib


def chromosome_bounds(chr_pos, n_windows):
    """int32 array of C + 1 window numbers: the sorted starts of ``chr_pos`` followed by ``n_windows``.

    ``ValueError`` for a start that is not an integer inside ``[0, n_windows)``, duplicate starts, an empty table or no
    chromosome starting at window 0 (every window belongs to exactly one chromosome)."""
    try:
        raw = list(chr_pos.values())
    except AttributeError:
        raise ValueError("tl.cnv_states: chr_pos must map chromosome names to their first window") from None
    if not raw:
        raise ValueError("tl.cnv_states: chr_pos is empty")
    starts = []
    for v in raw:
        try:
            i = int(v)
        except (TypeError, ValueError):
            raise ValueError(f"tl.cnv_states: chr_pos start {v!r} is not an integer") from None
        if isinstance(v, bool) or i != v:
            raise ValueError(f"tl.cnv_states: chr_pos start {v!r} is not an integer")
        if not 0 <= i < n_windows:
            raise ValueError(f"tl.cnv_states: chr_pos start {i} is outside [0, {n_windows})")
        starts.append(i)
    starts.sort()
    if any(a == b for a, b in zip(starts, starts[1:])):
        raise ValueError("tl.cnv_states: two chromosomes of chr_pos start at the same window")
    if starts[0] != 0:
        raise ValueError("tl.cnv_states: no chromosome of chr_pos starts at window 0")
    return np.asarray(starts + [int(n_windows)], dtype=np.int32)


def _positive(name, value):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"tl.cnv_states: {name}={value!r} must be a number") from None
    if isinstance(value, bool) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"tl.cnv_states: {name}={value!r} must be finite and > 0")
    return v


def check_emissions(who, key, x, m, amp, h, sig):
    """Rule 6 of DESIGN.md 4.13: ``ValueError`` when the emission of the stored value of the largest magnitude overflows.

    ``m`` is that magnitude, ``t = m + amp``; the state ``-amp`` forms this ``t`` for a positive value and the state
    ``+amp`` for a negative one, and no other ``t`` of the matrix is larger, so every emission ``-(t t) h`` is finite
    exactly when ``(t t) h`` is.  Without the check all three emissions of such a window are ``-inf``: the posteriors of
    its chromosome become 0 / 0 and the Viterbi chain calls it neutral.  The ``m`` of a ``PackedCsr`` covers the unused
    tail of its buffers; only where that fails the rule (or is NaN) are the stored entries looked at alone, which reads
    their number back."""
    def overflows(v):
        t = v + amp
        return not math.isfinite((t * t) * h)

    if not overflows(m):
        return
    if isinstance(x, _engine.PackedCsr):
        m = float(_engine.states_absmax(x.data[:x.nnz()]).item())
        if not overflows(m):
            return
    raise ValueError(f"{who}: sigma={sig!r} and amplitude={amp!r} overflow float64 on the value of magnitude {m!r} in "
                     f"{key}: (|x| + amplitude)^2 / (2 sigma^2) is not finite, so no state could be told from another; "
                     "rescale the matrix or clip the value")


def cnv_states(adata, use_rep="cnv", key_added="cnv_states", inplace=True, *, amplitude=None, sigma=None,
               switch_prob=1e-3, return_info=False):
    """Call every window of every cell lost (-1), neutral (0) or gained (+1).

    A three-state hidden Markov chain with Gaussian emissions of means ``(-amplitude, 0, +amplitude)`` and standard
    deviation ``sigma`` runs along each chromosome of each cell; the most likely path (Viterbi) is the call.  Chains never
    cross a chromosome boundary.  Requires running :func:`infercnvpy_amd.tl.infercnv` first.

    Parameters
    ----------
    adata
        annotated data matrix
    use_rep
        ``adata.obsm[f"X_{use_rep}"]`` (n x W) is called: a scipy CSR / CSC matrix, a dense host array, a
        :class:`infercnvpy_amd.PackedCsr` or a dense CUDA tensor.  Stored values are used as float64, an entry that is
        not stored is 0.0.  ``adata.uns[use_rep]["chr_pos"]`` holds the first window of every chromosome.
    key_added
        The calls go to ``adata.obsm[f"X_{key_added}"]`` (int8), the share of each cell's windows that are not neutral
        to ``adata.obs[key_added + "_fraction"]`` (float64: an integer count divided by W), the resolved parameters to
        ``adata.uns[key_added]["params"]``.
    inplace
        If True, store the result in adata, otherwise return ``(states, fraction)``.
    amplitude
        Mean of the gain state (the loss state has its negative); None: ``2 * sigma``.
    sigma
        Standard deviation of the emissions; None: the root mean square of the matrix over all n W windows,
        ``sqrt(S / (n W))`` with S the exactly rounded sum (``math.fsum``) of the per-cell sums of squares formed on
        the device.  An all-zero matrix (``sigma == 0``) gives all-neutral calls.
    switch_prob
        Probability of leaving a state between two windows, in (0, 1); each of the other two states gets half of it.
    return_info
        Also return a dict: ``amplitude``, ``sigma``, ``n_chromosomes`` and ``stage_ms`` (sums of squares, chains;
        host clocks, the second one waits for the kernel).

    Returns
    -------
    None when ``inplace`` (and not ``return_info``); else ``(states, fraction)``, followed by the info dict when
    ``return_info``.  Host input gives host numpy arrays.  Device input (``PackedCsr``, CUDA tensor) leaves ``states`` on
    the device as a CUDA int8 tensor; with ``inplace=False`` the fraction is a CUDA float64 tensor as well and the call
    returns without waiting for the chains, while ``inplace=True`` copies the n counts back for ``adata.obs``.  A
    non-finite value raises ``ValueError`` (one flag read back from the device before the chains are launched), and so
    does a finite one so large that its emission overflows: ``(|x| + amplitude)^2 / (2 sigma^2)`` must be finite for the
    stored value of the largest magnitude, which is read back with the flag.
    """
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"tl.cnv_states: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"tl.cnv_states: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    x = adata.obsm[key]
    if len(x.shape) != 2:
        raise ValueError("tl.cnv_states: X must be 2-D")
    n, w = int(x.shape[0]), int(x.shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"tl.cnv_states: empty matrix of shape {(n, w)}")
    if w > _lib.ICV_STATES_MAX_WINDOWS:
        raise ValueError(f"tl.cnv_states: {w} windows; the kernel keeps a cell's windows in LDS and takes at most "
                         f"{_lib.ICV_STATES_MAX_WINDOWS}")
    bounds = chromosome_bounds(adata.uns[use_rep]["chr_pos"], w)
    amp = None if amplitude is None else _positive("amplitude", amplitude)
    sig = None if sigma is None else _positive("sigma", sigma)
    try:
        p = float(switch_prob)
    except (TypeError, ValueError):
        raise ValueError(f"tl.cnv_states: switch_prob={switch_prob!r} must be a number") from None
    if isinstance(switch_prob, bool) or not 0.0 < p < 1.0:
        raise ValueError(f"tl.cnv_states: switch_prob={switch_prob!r} must lie in (0, 1)")
    stay, sw = math.log(1.0 - p), math.log(p / 2.0)
    if not (math.isfinite(stay) and math.isfinite(sw)):
        raise ValueError(f"tl.cnv_states: switch_prob={switch_prob!r} is too close to 0 or 1 for float64")

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    dm = _engine.states_input(x)
    t0 = time.perf_counter()
    q, flag = _engine.states_rowsq(dm)
    absmax = _engine.states_absmax(_engine.states_stored_values(dm))
    if sig is None:
        q_host = q.cpu().numpy()
    nonfinite, m = _engine.states_flag_and_absmax(flag, absmax)
    if nonfinite:
        raise ValueError(f"tl.cnv_states: {key} has non-finite values")
    if sig is None:
        try:
            sig = math.sqrt(math.fsum(q_host.tolist()) / (float(n) * float(w)))
        except OverflowError:
            sig = math.inf
        if not math.isfinite(sig):
            raise ValueError(f"tl.cnv_states: the default sigma of {key} overflows float64; pass sigma")
    if amp is None:
        amp = 2.0 * sig
    t1 = time.perf_counter()
    with torch.cuda.device(dm.device):
        if sig == 0.0:  # an all-zero matrix: nothing to call
            states = torch.zeros((n, w), dtype=torch.int8, device="cuda")
            count = torch.zeros(n, dtype=torch.int32, device="cuda")
        else:
            h = 1.0 / (2.0 * sig * sig)
            if not (math.isfinite(h) and h > 0.0 and math.isfinite(amp) and amp > 0.0):
                raise ValueError(f"tl.cnv_states: sigma={sig!r} / amplitude={amp!r} leave float64's range "
                                 "(1 / (2 sigma^2) must be finite and > 0)")
            check_emissions("tl.cnv_states", key, x, m, amp, h, sig)
            states, count = _engine.states_viterbi(dm, bounds, amplitude=amp, h=h, stay=stay, sw=sw)
        info = None
        if return_info:
            torch.cuda.current_stream().synchronize()
            info = {"amplitude": amp, "sigma": sig, "n_chromosomes": int(bounds.shape[0]) - 1,
                    "stage_ms": {"rowsq": (t1 - t0) * 1e3, "viterbi": (time.perf_counter() - t1) * 1e3}}
        if on_device and not inplace:
            fraction = _engine.states_fraction(count, w)
        else:
            fraction = count.cpu().numpy().astype(np.float64) / float(w)
        if not on_device:
            states = states.cpu().numpy()
    if inplace:
        adata.obsm[f"X_{key_added}"] = states
        adata.obs[key_added + "_fraction"] = fraction
        adata.uns[key_added] = {"params": {"amplitude": amp, "sigma": sig, "switch_prob": p}}
        return (states, fraction, info) if return_info else None
    return (states, fraction, info) if return_info else (states, fraction)

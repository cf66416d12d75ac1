"""The model of the hidden Markov chains, resolved once for ``tl.cnv_states``, ``tl.cnv_posteriors`` and
``tl.cnv_states_fit`` (three states) and for ``tl.cnv_copy_states``, ``tl.cnv_copy_posteriors`` and
``tl.cnv_copy_states_fit`` (K states).

The functions of a family must derive the same ``(amplitude, sigma, switch_prob)`` from the same matrix and the same
arguments (DESIGN.md 4.13 rules 1 and 6), otherwise the posteriors do not belong to the calls and the fit does not start
where the calls were made.  :func:`resolve` is that derivation; what differs between the callers is an argument of it.
:func:`resolve_levels` adds the ``levels`` of the K-state model.  The argument checks that the functions
downstream of the calls share live here too: :func:`chromosome_bounds`, :func:`at_least_one` and :func:`call_matrix`.
"""
from __future__ import annotations

import math
import sys
import time
from typing import NamedTuple

import numpy as np

from .. import _engine

MIN_STATES, MAX_STATES = 2, 8  # of the K-state model
DEFAULT_STEPS = (-2, -1, 0, 1, 2, 3)  # complete loss, one-copy loss, neutral, one-, two-copy and a higher gain


def chromosome_bounds(chr_pos, n_windows, who="tl.cnv_states"):
    """int32 array of C + 1 window numbers: the sorted starts of ``chr_pos`` followed by ``n_windows``.

    ``ValueError`` for a start that is not an integer inside ``[0, n_windows)``, duplicate starts, an empty table or no
    chromosome starting at window 0 (every window belongs to exactly one chromosome); ``who`` prefixes the message."""
    try:
        raw = list(chr_pos.values())
    except AttributeError:
        raise ValueError(f"{who}: chr_pos must map chromosome names to their first window") from None
    if not raw:
        raise ValueError(f"{who}: chr_pos is empty")
    starts = []
    for v in raw:
        try:
            i = int(v)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: chr_pos start {v!r} is not an integer") from None
        if isinstance(v, bool) or i != v:
            raise ValueError(f"{who}: chr_pos start {v!r} is not an integer")
        if not 0 <= i < n_windows:
            raise ValueError(f"{who}: chr_pos start {i} is outside [0, {n_windows})")
        starts.append(i)
    starts.sort()
    if any(a == b for a, b in zip(starts, starts[1:])):
        raise ValueError(f"{who}: two chromosomes of chr_pos start at the same window")
    if starts[0] != 0:
        raise ValueError(f"{who}: no chromosome of chr_pos starts at window 0")
    return np.asarray(starts + [int(n_windows)], dtype=np.int32)


def _positive(name, value, who="tl.cnv_states"):
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name}={value!r} must be a number") from None
    if isinstance(value, bool) or not (math.isfinite(v) and v > 0):
        raise ValueError(f"{who}: {name}={value!r} must be finite and > 0")
    return v


def unit_fraction(who, name, value):
    """``value`` as an exact ``fractions.Fraction`` (a float is taken at its binary value); ``ValueError`` unless it is a
    number in (0, 1]."""
    from fractions import Fraction

    try:
        f = Fraction(value) if isinstance(value, (int, str, Fraction)) else Fraction(float(value))
    except (TypeError, ValueError, OverflowError, ZeroDivisionError):
        raise ValueError(f"{who}: {name}={value!r} must be a number in (0, 1]") from None
    if isinstance(value, bool) or not 0 < f <= 1:
        raise ValueError(f"{who}: {name}={value!r} must lie in (0, 1]")
    return f


def at_least_one(who, name, value):
    """``value`` as an int; ``ValueError`` unless it is an integer >= 1."""
    try:
        k = int(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{who}: {name}={value!r} must be an integer >= 1") from None
    if isinstance(value, bool) or k != value or k < 1:
        raise ValueError(f"{who}: {name}={value!r} must be an integer >= 1")
    return k


def call_matrix(adata, who, key, cnv_key, chr_pos_hint, pkey=None):
    """(x, post, n, w): the int8 call matrix ``adata.obsm[key]`` of ``tl.cnv_segments`` and ``tl.cnv_states_filter`` after
    its checks, in the order they are reported: the keys, 2-D, int8, not empty.  ``chr_pos_hint`` ends the message about a
    missing ``adata.uns[cnv_key]["chr_pos"]``.  With ``pkey``, ``post = adata.obsm[pkey]`` must be there (looked for after
    ``key``) and be float64 of the same shape (checked before the empty matrix); otherwise ``post`` is None."""
    if key not in adata.obsm:
        raise KeyError(f"{who}: {key} not found in adata.obsm. Did you run `tl.cnv_states`?")
    if pkey is not None and pkey not in adata.obsm:
        raise KeyError(f"{who}: {pkey} not found in adata.obsm. Did you run `tl.cnv_posteriors`?")
    if cnv_key not in adata.uns or "chr_pos" not in adata.uns[cnv_key]:
        raise KeyError(f"{who}: chr_pos not found in adata.uns['{cnv_key}']. Did you run {chr_pos_hint}")
    x, post = adata.obsm[key], None if pkey is None else adata.obsm[pkey]
    shape = getattr(x, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError(f"{who}: {key} must be 2-D")
    if str(getattr(x, "dtype", None)) not in ("int8", "torch.int8"):
        raise ValueError(f"{who}: {key} must be int8 (-1 loss, 0 neutral, +1 gain), not "
                         f"{getattr(x, 'dtype', type(x).__name__)}")
    if pkey is not None:
        if tuple(getattr(post, "shape", ())) != tuple(shape):
            raise ValueError(f"{who}: {pkey} has shape {tuple(getattr(post, 'shape', ()))}, {key} has {tuple(shape)}")
        if str(getattr(post, "dtype", None)) not in ("float64", "torch.float64"):
            raise ValueError(f"{who}: {pkey} must be float64, not {getattr(post, 'dtype', type(post).__name__)}")
    n, w = int(shape[0]), int(shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{who}: empty matrix of shape {(n, w)}")
    return x, post, n, w


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


class Model(NamedTuple):
    """What :func:`resolve` returns."""
    x: object          # adata.obsm[key], as it was stored
    n: int
    w: int
    bounds: np.ndarray  # chromosome_bounds
    dm: object         # the DeviceMatrix of x
    on_device: bool    # x was a PackedCsr or a CUDA tensor
    amp: float
    sig: float
    p: float
    qs: float | None   # the sum of squares of the matrix, where it was formed
    m: float           # the largest magnitude of a stored value
    h: float | None    # 1 / (2 sigma^2); None for sigma == 0 (an all-zero matrix)
    t0: float          # time.perf_counter() before and after the sums of squares and their read-back
    t1: float
    rest: object       # what then() returned


def resolve(adata, use_rep, who, *, max_windows, keeps, amplitude, sigma, switch_prob, log_switch, sum_of_squares,
            zero_model=False, then=None, default_sigma=None, n_states=3):
    """The common opening of the chain functions: arguments checked, matrix on the device, model resolved.

    who
        The caller's name; it prefixes every message.
    max_windows, keeps
        The kernel's window cap and what it keeps in LDS, for the cap's message.
    amplitude, sigma, switch_prob
        As the caller got them; ``switch_prob`` is not None.
    log_switch
        True: ``switch_prob`` is too close to 0 or 1 when ``log(1 - p)`` or ``log(p / 2)`` is not finite or the share
        ``p / (n_states - 1)`` of one other state is 0 (the Viterbi chain adds logarithms).  False: when that share (at
        most ``p / 2``) is not a normal float64 or ``1 - p`` is not in (0, 1) (the forward-backward chain multiplies
        probabilities).
    sum_of_squares
        True: the per-row sums of squares are always read back and their sum must be finite.  False: only for the
        default ``sigma``; with ``sigma`` given the one pair (non-finite flag, largest magnitude) is all that is read.
    zero_model
        ``amplitude`` and ``sigma`` are the 0.0 that ``tl.cnv_states`` stores for an all-zero matrix: taken as they are.
    then
        Called after the model's arguments are checked and before anything touches the device: the caller's checks of
        its remaining arguments.  What it returns is ``Model.rest``.
    default_sigma
        None, or ``default_sigma(dm, bounds, rms)``: the caller's own default for a ``sigma`` of None, given the root
        mean square that is the default otherwise.
    n_states
        The K of the model: each of the other K - 1 states gets an equal share of ``switch_prob``.  (The K-state
        functions used to test that share in ``then()``, which has always run right after the test here: one test in
        its place reports the same faults in the same order.)

    Raises in this order: keys, shape, cap, ``chr_pos``, ``amplitude``, ``sigma``, ``switch_prob``, ``then()``, and
    only then what needs the device (non-finite values, overflows)."""
    key = f"X_{use_rep}"
    if key not in adata.obsm:
        raise KeyError(f"{who}: {key} not found in adata.obsm. Did you run `tl.infercnv`?")
    if use_rep not in adata.uns or "chr_pos" not in adata.uns[use_rep]:
        raise KeyError(f"{who}: chr_pos not found in adata.uns['{use_rep}']. Did you run `tl.infercnv`?")
    x = adata.obsm[key]
    if len(x.shape) != 2:
        raise ValueError(f"{who}: X must be 2-D")
    n, w = int(x.shape[0]), int(x.shape[1])
    if n < 1 or w < 1:
        raise ValueError(f"{who}: empty matrix of shape {(n, w)}")
    if w > max_windows:
        raise ValueError(f"{who}: {w} windows; the kernel keeps {keeps} in LDS and takes at most {max_windows}")
    bounds = chromosome_bounds(adata.uns[use_rep]["chr_pos"], w)
    if zero_model:
        amp, sig = 0.0, 0.0
    else:
        amp = None if amplitude is None else _positive("amplitude", amplitude, who)
        sig = None if sigma is None else _positive("sigma", sigma, who)
    try:
        p = float(switch_prob)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: switch_prob={switch_prob!r} must be a number") from None
    if isinstance(switch_prob, bool) or not 0.0 < p < 1.0:
        raise ValueError(f"{who}: switch_prob={switch_prob!r} must lie in (0, 1)")
    share = p / max(2, n_states - 1)
    if log_switch:
        in_range = math.isfinite(math.log(1.0 - p)) and math.isfinite(math.log(p / 2.0)) and share > 0.0
    else:
        in_range = share >= sys.float_info.min and 0.0 < 1.0 - p < 1.0
    if not in_range:
        raise ValueError(f"{who}: switch_prob={switch_prob!r} is too close to 0 or 1 for float64")
    rest = None if then is None else then()

    torch = _engine._torch()
    on_device = isinstance(x, (_engine.PackedCsr, torch.Tensor))
    dm = _engine.matrix_input(x, who)
    t0 = time.perf_counter()
    q, flag = _engine.states_rowsq(dm)
    absmax = _engine.states_absmax(_engine.states_stored_values(dm))
    want_q = sum_of_squares or sig is None
    if want_q:
        q_host = q.cpu().numpy()
    nonfinite, m = _engine.flag_and_absmax(flag, absmax)
    if nonfinite:
        raise ValueError(f"{who}: {key} has non-finite values")
    qs = None
    if want_q:
        try:
            qs = math.fsum(q_host.tolist())
        except OverflowError:
            qs = math.inf
        if sig is None:
            sig = math.sqrt(qs / (float(n) * float(w)))
            if default_sigma is not None and math.isfinite(sig):
                sig = default_sigma(dm, bounds, sig)
        if not (math.isfinite(qs) and math.isfinite(sig)):
            raise ValueError(f"{who}: the sum of squares of {key} overflows float64" if sum_of_squares else
                             f"{who}: the default sigma of {key} overflows float64; pass sigma")
    if amp is None:
        amp = 2.0 * sig
    t1 = time.perf_counter()
    h = None
    if sig != 0.0:
        h = 1.0 / (2.0 * sig * sig)
        if not (math.isfinite(h) and h > 0.0 and math.isfinite(amp) and amp > 0.0):
            raise ValueError(f"{who}: sigma={sig!r} / amplitude={amp!r} leave float64's range "
                             "(1 / (2 sigma^2) must be finite and > 0)")
        check_emissions(who, key, x, m, amp, h, sig)
    return Model(x, n, w, bounds, dm, on_device, amp, sig, p, qs, m, h, t0, t1, rest)


def check_levels(levels, who="tl.cnv_copy_states"):
    """(list of K floats with the neutral one as ``0.0``, its index z); ``ValueError`` unless ``levels`` are K finite
    numbers, 2 <= K <= 8, strictly ascending, exactly one of them zero (``-0.0`` counts as a zero)."""
    try:
        out = [float(v) for v in levels]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: levels={levels!r} must be a sequence of numbers") from None
    if not MIN_STATES <= len(out) <= MAX_STATES:
        raise ValueError(f"{who}: levels has {len(out)} states; the chain takes {MIN_STATES} to {MAX_STATES}")
    if not all(math.isfinite(v) for v in out):
        raise ValueError(f"{who}: levels={out!r} must be finite")
    if any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError(f"{who}: levels={out!r} must ascend strictly")
    zeros = [k for k, v in enumerate(out) if v == 0.0]
    if len(zeros) != 1:
        raise ValueError(f"{who}: levels={out!r} must hold exactly one 0.0, the neutral state")
    out[zeros[0]] = 0.0
    return out, zeros[0]


def resolve_levels(adata, use_rep, who, *, levels, amplitude, sigma, switch_prob, log_switch, max_windows, keeps,
                   zero_levels=None):
    """The common opening of ``tl.cnv_copy_states`` and ``tl.cnv_copy_posteriors``: ``(mo, mu, z, k)`` with ``mo`` the
    :class:`Model` of :func:`resolve`, ``mu`` the K state means and ``z`` the index of the neutral one.

    ``max_windows(k)`` and ``keeps(k)`` give :func:`resolve` the kernel's cap and its words for K states.
    ``zero_levels``: the ``(mu, z)`` that ``tl.cnv_copy_states`` stored for an all-zero matrix (its levels are all 0),
    taken as they are, with ``zero_model`` for :func:`resolve`.

    Raises in this order: ``levels`` together with ``amplitude``, :func:`check_levels`, what :func:`resolve` raises, and
    for the default levels ``[k * amplitude for k in DEFAULT_STEPS]`` their own :func:`check_levels` and
    :func:`check_emissions`.  Rule 6 with given levels is the check of :func:`resolve` itself under the amplitude
    ``max(|levels[0]|, |levels[-1]|)``."""
    if levels is not None and amplitude is not None:
        raise ValueError(f"{who}: levels and amplitude are both given; amplitude only spaces the default levels")
    if zero_levels is not None:
        mu, z = zero_levels
    else:
        mu, z = (None, None) if levels is None else check_levels(levels, who)
    k = len(DEFAULT_STEPS) if mu is None else len(mu)
    mo = resolve(adata, use_rep, who, max_windows=max_windows(k), keeps=keeps(k),
                 amplitude=amplitude if mu is None else max(abs(mu[0]), abs(mu[-1])), sigma=sigma,
                 switch_prob=switch_prob, log_switch=log_switch, sum_of_squares=False,
                 zero_model=zero_levels is not None, n_states=k)
    if mu is None:
        mu = [float(s) * mo.amp for s in DEFAULT_STEPS]
        z = DEFAULT_STEPS.index(0)
        if mo.h is not None:
            mu, z = check_levels(mu, who)
            check_emissions(who, f"X_{use_rep}", mo.x, mo.m, max(abs(mu[0]), abs(mu[-1])), mo.h, mo.sig)
    return mo, mu, z, k

"""The arguments of tl.cnv_states, tl.cnv_posteriors and tl.cnv_states_fit that are refused before any GPU work: for every
bad input the exception's type and its whole message.  The three functions share one resolver (tl/_hmm.py); the strings
below are what each function raised when it still had its own copy of these checks, so the table holds the resolver to
them character for character.  The one change: a bad amplitude or sigma of tl.cnv_states_fit is reported under that
function's name, where it used to say tl.cnv_states.  No test here needs a device."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

CAPS = {"cnv_states": 16384, "cnv_posteriors": 4096, "cnv_states_fit": 4096}

# tl.cnv_states tests switch_prob by its logarithms, which are finite for every float64 p in (0, 1) whose half is not 0;
# for the one p whose half is 0, math.log raises, in the interpreter's words
try:
    math.log(0.0)
except ValueError as e:
    LOG_OF_ZERO = str(e)


def _adata(n=4, w=10, chr_pos=None, x=None):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def _no_chr_pos():
    ad = _adata()
    del ad.uns["cnv"]["chr_pos"]
    return ad


def _cases(fn):
    """(id, () -> adata, keywords) of every bad input of the function ``fn``."""
    cap = CAPS[fn]
    out = [
        ("missing obsm key", _adata, {"use_rep": "other"}),
        ("missing chr_pos", _no_chr_pos, {}),
        ("1-D X", lambda: _adata(x=np.ones(4)), {}),
        ("empty shape", lambda: _adata(x=np.ones((4, 0))), {}),
        ("W above the cap", lambda: _adata(n=1, x=sp.csr_matrix((1, cap + 1)), chr_pos={"chr1": 0}), {}),
    ]
    for cid, chr_pos in [
        ("chr_pos outside", {"chr1": 0, "chr2": 10}), ("chr_pos negative", {"chr1": 0, "chr2": -1}),
        ("chr_pos same window", {"chr1": 0, "chr2": 4, "chr3": 4}), ("chr_pos not at 0", {"chr1": 1, "chr2": 4}),
        ("chr_pos fraction", {"chr1": 0, "chr2": 2.5}), ("chr_pos string", {"chr1": 0, "chr2": "x"}),
        ("chr_pos empty", {}), ("chr_pos list", [0, 4]),
    ]:
        out.append((cid, (lambda c=chr_pos: _adata(chr_pos=c)), {}))
    for name in ("amplitude", "sigma"):
        for v in (0, -1, float("nan"), float("inf"), True, "x"):
            out.append((f"{name}={v!r}", _adata, {name: v}))
    # the last one lies in (0, 1) and is too close to 0 for the function's own test
    for v in (0, 1, True, "x", 5e-324 if fn == "cnv_states" else 1e-320):
        out.append((f"switch_prob={v!r}", _adata, {"switch_prob": v}))
    return out


EXPECTED = {
    "cnv_states": {
        'missing obsm key': (KeyError, 'tl.cnv_states: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_states: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_states: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_states: empty matrix of shape (4, 0)'),
        'W above the cap': (ValueError, "tl.cnv_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_states: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_states: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_states: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_states: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_states: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_states: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_states: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_states: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_states: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_states: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_states: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_states: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_states: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_states: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_states: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_states: switch_prob='x' must be a number"),
        'switch_prob=5e-324': (ValueError, LOG_OF_ZERO),
    },
    "cnv_posteriors": {
        'missing obsm key': (KeyError, 'tl.cnv_posteriors: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_posteriors: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_posteriors: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_posteriors: empty matrix of shape (4, 0)'),
        'W above the cap': (ValueError, "tl.cnv_posteriors: 4097 windows; the kernel keeps a cell's windows and forward variables in LDS and takes at most 4096"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_posteriors: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_posteriors: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_posteriors: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_posteriors: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_posteriors: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_posteriors: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_posteriors: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_posteriors: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_posteriors: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_posteriors: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_posteriors: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_posteriors: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_posteriors: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_posteriors: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_posteriors: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_posteriors: switch_prob='x' must be a number"),
        'switch_prob=1e-320': (ValueError, 'tl.cnv_posteriors: switch_prob=1e-320 is too close to 0 or 1 for float64'),
    },
    "cnv_states_fit": {
        'missing obsm key': (KeyError, 'tl.cnv_states_fit: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_states_fit: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_states_fit: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_states_fit: empty matrix of shape (4, 0)'),
        'W above the cap': (ValueError, "tl.cnv_states_fit: 4097 windows; the kernel keeps a cell's windows and forward variables in LDS and takes at most 4096"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_states_fit: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_states_fit: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_states_fit: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_states_fit: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_states_fit: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_states_fit: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_states_fit: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_states_fit: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_states_fit: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_states_fit: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_states_fit: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_states_fit: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_states_fit: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_states_fit: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_states_fit: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_states_fit: switch_prob='x' must be a number"),
        'switch_prob=1e-320': (ValueError, 'tl.cnv_states_fit: switch_prob=1e-320 is too close to 0 or 1 for float64'),
    },
}


def test_the_window_caps_are_the_librarys():
    from infercnvpy_amd import _lib

    assert CAPS == {"cnv_states": _lib.ICV_STATES_MAX_WINDOWS, "cnv_posteriors": _lib.ICV_POSTERIOR_MAX_WINDOWS,
                    "cnv_states_fit": _lib.ICV_POSTERIOR_MAX_WINDOWS}


@pytest.mark.parametrize("fn", list(EXPECTED))
def test_every_bad_input_keeps_its_exception_and_its_whole_message(fn):
    import infercnvpy_amd as cnv

    cases = _cases(fn)
    assert [cid for cid, _, _ in cases] == list(EXPECTED[fn])
    for cid, make, kw in cases:
        kind, message = EXPECTED[fn][cid]
        with pytest.raises(kind) as info:
            getattr(cnv.tl, fn)(make(), **kw)
        assert type(info.value) is kind, (fn, cid)
        assert info.value.args[0] == message, (fn, cid)


# one input that is wrong in two ways: keys, shape, cap, chr_pos, amplitude, sigma, switch_prob, then the function's
# own arguments, and only then the device
ORDER = [
    (lambda: _adata(x=np.ones(4)), {"use_rep": "other"}, KeyError, "X_other not found"),
    (lambda: _adata(n=1, x=sp.csr_matrix((1, 16385)), chr_pos={}), {}, ValueError, "16385 windows"),
    (lambda: _adata(chr_pos={}), {"amplitude": 0}, ValueError, "chr_pos is empty"),
    (_adata, {"amplitude": 0, "sigma": 0}, ValueError, "amplitude=0 must be finite and > 0"),
    (_adata, {"sigma": 0, "switch_prob": 0}, ValueError, "sigma=0 must be finite and > 0"),
]


@pytest.mark.parametrize("fn", list(EXPECTED))
def test_the_first_fault_in_the_order_of_the_checks_is_the_one_reported(fn):
    import infercnvpy_amd as cnv

    for make, kw, kind, part in ORDER:
        with pytest.raises(kind) as info:
            getattr(cnv.tl, fn)(make(), **kw)
        assert part in info.value.args[0], (fn, part)


@pytest.mark.parametrize("kw, message", [
    ({"switch_prob": 0, "fit": "nope"}, "tl.cnv_states_fit: switch_prob=0 must lie in (0, 1)"),
    ({"fit": "nope"}, "tl.cnv_states_fit: fit=('nope',) must be a non-empty subset of "
                      "('amplitude', 'sigma', 'switch_prob')"),
    ({"fit": 3}, "tl.cnv_states_fit: fit=3 must be a sequence of parameter names"),
    ({"fit": (), "max_iter": 0}, "tl.cnv_states_fit: fit=() must be a non-empty subset of "
                                 "('amplitude', 'sigma', 'switch_prob')"),
    ({"max_iter": 0, "tol": -1}, "tl.cnv_states_fit: max_iter=0 must be an int >= 1"),
    ({"max_iter": True}, "tl.cnv_states_fit: max_iter=True must be an int >= 1"),
    ({"tol": "x"}, "tl.cnv_states_fit: tol='x' must be a number"),
    ({"tol": -1}, "tl.cnv_states_fit: tol=-1 must be finite and >= 0"),
])
def test_the_fits_own_arguments_are_checked_after_the_models_and_before_the_device(kw, message):
    import infercnvpy_amd as cnv

    with pytest.raises(ValueError) as info:
        cnv.tl.cnv_states_fit(_adata(), **kw)
    assert str(info.value) == message


def test_the_helpers_of_tl_states_are_those_of_tl_hmm():
    from infercnvpy_amd.tl import _hmm, _posteriors, _states

    assert _states.chromosome_bounds is _hmm.chromosome_bounds
    assert _states.check_emissions is _hmm.check_emissions
    assert _states._positive is _hmm._positive
    assert not hasattr(_posteriors, "_positive")  # (there is no second one)

"""The arguments of tl.cnv_copy_states, tl.cnv_copy_posteriors, tl.cnv_copy_states_fit and tl.cnv_copy_states_filter, and of
the four icv_copy_* entry points, that are refused before any GPU work: for every bad input the exception's type (the
entry's status) and its whole message, and for inputs with two faults the one that is reported.  The strings below are
what the functions raised while each still carried its own copy of the checks they now share (tl/_hmm.py, by_states and
the one model struct of csrc/icv_api.hip), so the tables hold the shared code to them character for character.  No test
here needs a device."""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp

LDS = 163840
INVALID, UNSUPPORTED = 1, 2  # ICV_ERR_INVALID, ICV_ERR_UNSUPPORTED
FILTER_CAP = 1 << 22
EIGHT = [0.1 * s for s in range(-3, 5)]  # K = 8 levels
EIGHT_STEPS = tuple(range(-3, 5))

# tl.cnv_copy_states tests switch_prob by its logarithms; for the one p whose half is 0, math.log raises, in the
# interpreter's words
try:
    math.log(0.0)
except ValueError as e:
    LOG_OF_ZERO = str(e)


def chain_cap(k):
    return LDS // (8 * (k + 1))


def stats_cap(k, n_chr):
    return max(LDS - 8 * (2 * k + 1) * n_chr, 0) // (8 * (k + 1))


def test_the_window_caps_are_the_librarys():
    from infercnvpy_amd import _lib

    assert _lib.ICV_COPY_POSTERIOR_LDS_BYTES == LDS and _lib.ICV_FILTER_MAX_WINDOWS == FILTER_CAP
    assert _lib.ICV_COPY_STATES_MAX_WINDOWS == 16384
    assert (_lib.ICV_ERR_INVALID, _lib.ICV_ERR_UNSUPPORTED) == (INVALID, UNSUPPORTED)
    for k in range(2, 9):
        assert _lib.ICV_COPY_POSTERIOR_MAX_WINDOWS(k) == chain_cap(k)
        for n_chr in (1, 23, 2000):
            assert _lib.ICV_COPY_POSTERIOR_STATS_MAX_WINDOWS(k, n_chr) == stats_cap(k, n_chr)


# ---- the three chain functions -----------------------------------------------------------------------------------------------
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


def _wide(w, n_chr=1):
    """One row of w windows in n_chr chromosomes, nothing stored."""
    return lambda: _adata(n=1, x=sp.csr_matrix((1, w)), chr_pos={f"chr{c}": c for c in range(n_chr)})


def _stored(params):
    """An adata where tl.cnv_copy_states left ``params``."""
    def make():
        ad = _adata()
        ad.uns["cnv_copy_states"] = {"params": params}
        return ad
    return make


def _chain_cases(fn):
    """(id, () -> adata, keywords) of every bad input of the chain function ``fn``."""
    fit = fn == "cnv_copy_states_fit"
    eight = {"steps": EIGHT_STEPS} if fit else {"levels": EIGHT}
    two = {"steps": (0, 1)} if fit else {"levels": (0.0, 0.3)}
    cap = {"cnv_copy_states": lambda k: 16384, "cnv_copy_posteriors": chain_cap,
           "cnv_copy_states_fit": lambda k: stats_cap(k, 1)}[fn]
    out = [
        ("missing obsm key", _adata, {"use_rep": "other"}),
        ("missing chr_pos", _no_chr_pos, {}),
        ("1-D X", lambda: _adata(x=np.ones(4)), {}),
        ("empty shape", lambda: _adata(x=np.ones((4, 0))), {}),
        ("W above the cap, K = 6", _wide(cap(6) + 1), {}),
        ("W above the cap, K = 8", _wide(cap(8) + 1), eight),
        ("W above the cap, K = 2", _wide(cap(2) + 1), two),
    ]
    if fit:  # under the cap of one chromosome, above the cap of 23 and of 2000
        out += [("W above the cap of 23 chromosomes", _wide(stats_cap(6, 23) + 1, 23), {}),
                ("W above the cap of 23 chromosomes, K = 8", _wide(stats_cap(8, 23) + 1, 23), eight),
                ("2000 chromosomes fill the LDS, K = 8", _wide(2000, 2000), eight)]
    for cid, chr_pos in [
        ("chr_pos outside", {"chr1": 0, "chr2": 10}), ("chr_pos negative", {"chr1": 0, "chr2": -1}),
        ("chr_pos same window", {"chr1": 0, "chr2": 4, "chr3": 4}), ("chr_pos not at 0", {"chr1": 1, "chr2": 4}),
        ("chr_pos fraction", {"chr1": 0, "chr2": 2.5}), ("chr_pos string", {"chr1": 0, "chr2": "x"}),
        ("chr_pos bool", {"chr1": 0, "chr2": True}), ("chr_pos empty", {}), ("chr_pos list", [0, 4]),
    ]:
        out.append((cid, (lambda c=chr_pos: _adata(chr_pos=c)), {}))
    for name in ("amplitude", "sigma"):
        for v in (0, -1, float("nan"), float("inf"), True, "x"):
            out.append((f"{name}={v!r}", _adata, {name: v}))
    # in (0, 1) and too close to 0 for the function's own test.  tl.cnv_copy_states adds logarithms: 1e-323 passes with
    # p / 2 and fails with p / (K - 1) for K = 8 and K = 6; with K = 3 and K = 2 it is taken (the next fault is reported).
    # The others multiply probabilities: a p whose 1 - p rounds to 1 is refused whatever K is, and every other p in
    # (0, 1) has a normal p / (K - 1)
    log_test = fn == "cnv_copy_states"
    for v in (0, 1, True, "x", 5e-324 if log_test else 1e-320):
        out.append((f"switch_prob={v!r}", _adata, {"switch_prob": v}))
    p8 = 1e-323 if log_test else 1e-17
    three = {"steps": (-1, 0, 1)} if fit else {"levels": (-0.3, 0.0, 0.3)}
    out.append((f"switch_prob={p8!r}, K = 8", _adata, dict(eight, switch_prob=p8)))
    out.append((f"switch_prob={p8!r}, K = 6", _adata, {"switch_prob": p8}))
    out.append((f"switch_prob={p8!r}, K = 3, then sigma", _adata, dict(three, switch_prob=p8, sigma=0)))
    out.append((f"switch_prob={p8!r}, K = 2, then sigma", _adata, dict(two, switch_prob=p8, sigma=0)))
    if not log_test:  # the smallest p with 1 - p < 1 is taken with every K
        out.append(("switch_prob=2e-16, K = 8, then sigma", _adata, dict(eight, switch_prob=2e-16, sigma=0)))
    if fit:
        for cid, steps in [("steps not a sequence", 5), ("steps string", "ab"), ("steps fraction", (0, 1.5)),
                           ("steps bool", (0, True)), ("steps none", (0, None)), ("steps of one", (0,)),
                           ("steps of nine", tuple(range(9))), ("steps descend", (0, 2, 1)), ("steps repeat", (0, 1, 1)),
                           ("steps without 0", (1, 2, 3))]:
            out.append((cid, _adata, {"steps": steps}))
        for cid, kw in [("fit unknown", {"fit": "nope"}), ("fit not a sequence", {"fit": 3}), ("fit empty", {"fit": ()}),
                        ("max_iter=0", {"max_iter": 0}), ("max_iter=True", {"max_iter": True}),
                        ("max_iter=2.0", {"max_iter": 2.0}), ("tol='x'", {"tol": "x"}), ("tol=-1", {"tol": -1}),
                        ("tol=nan", {"tol": float("nan")}), ("tol=True", {"tol": True})]:
            out.append((cid, _adata, kw))
    else:
        out.append(("levels with amplitude", _adata, {"levels": (-0.3, 0.0, 0.3), "amplitude": 0.3}))
        for cid, levels in [("levels not a sequence", 5), ("levels string", "ab"), ("levels none", (0.0, None)),
                            ("levels of one", (0.0,)), ("levels of nine", [0.1 * s for s in range(9)]),
                            ("levels nan", (-0.3, 0.0, float("nan"))), ("levels inf", (-0.3, 0.0, float("inf"))),
                            ("levels descend", (0.0, 0.5, 0.3)), ("levels repeat", (0.0, 0.3, 0.3)),
                            ("levels two zeros", (-0.0, 0.0, 0.3)), ("levels without 0", (0.1, 0.2, 0.3))]:
            out.append((cid, _adata, {"levels": levels}))
    if fn == "cnv_copy_posteriors":
        ok = {"levels": [-0.3, 0.0, 0.3], "neutral": 1, "sigma": 0.1, "switch_prob": 1e-3}
        out += [("stored levels without 0", _stored(dict(ok, levels=[0.1, 0.2])), {}),
                ("stored sigma", _stored(dict(ok, sigma=-1.0)), {}),
                ("stored switch_prob", _stored(dict(ok, switch_prob=2.0)), {}),
                ("stored K = 8 above its cap", _wide_stored, {})]
    return out


def _wide_stored():
    ad = _wide(chain_cap(8) + 1)()
    ad.uns["cnv_copy_states"] = {"params": {"levels": EIGHT, "neutral": 3, "sigma": 0.1, "switch_prob": 1e-3}}
    return ad


# one input that is wrong in two ways: levels with amplitude, levels / steps, keys, shape, cap, chr_pos, amplitude, sigma,
# switch_prob (with its share of K - 1 states), then the function's own arguments, and only then the device
def _order_cases(fn):
    fit = fn == "cnv_copy_states_fit"
    eight = {"steps": EIGHT_STEPS} if fit else {"levels": EIGHT}
    p8 = 1e-323 if fn == "cnv_copy_states" else 1e-17
    out = [
        ("keys before shape", lambda: _adata(x=np.ones(4)), {"use_rep": "other"}),
        ("cap before chr_pos", lambda: _adata(n=1, x=sp.csr_matrix((1, 16385)), chr_pos={}), {}),
        ("chr_pos before amplitude", lambda: _adata(chr_pos={}), {"amplitude": 0}),
        ("amplitude before sigma", _adata, {"amplitude": 0, "sigma": 0}),
        ("sigma before switch_prob", _adata, {"sigma": 0, "switch_prob": 0}),
        ("sigma before switch_prob, K = 8", _adata, dict(eight, sigma=0, switch_prob=p8)),
    ]
    if fit:
        out += [("steps before keys", _adata, {"steps": (1, 2), "use_rep": "other"}),
                ("switch_prob before fit", _adata, {"switch_prob": 0, "fit": "nope"}),
                ("switch_prob before the cap of the chromosomes", _wide(stats_cap(8, 23) + 1, 23),
                 dict(eight, switch_prob=p8)),
                ("the cap of the chromosomes before fit", _wide(stats_cap(6, 23) + 1, 23), {"fit": "nope"}),
                ("fit before max_iter", _adata, {"fit": (), "max_iter": 0}),
                ("max_iter before tol", _adata, {"max_iter": 0, "tol": -1})]
    else:
        out += [("levels with amplitude before levels", _adata, {"levels": (1.0,), "amplitude": 0}),
                ("levels before keys", _adata, {"levels": (0.1, 0.2), "use_rep": "other"}),
                ("the cap is that of the given K", _wide(chain_cap(8) + 1 if fn == "cnv_copy_posteriors" else 16385),
                 dict(eight, sigma=0))]
    return out


CHAIN = ("cnv_copy_states", "cnv_copy_posteriors", "cnv_copy_states_fit")

EXPECTED = {
    'cnv_copy_states': {
        'missing obsm key': (KeyError, 'tl.cnv_copy_states: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_copy_states: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_copy_states: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_copy_states: empty matrix of shape (4, 0)'),
        'W above the cap, K = 6': (ValueError, "tl.cnv_copy_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
        'W above the cap, K = 8': (ValueError, "tl.cnv_copy_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
        'W above the cap, K = 2': (ValueError, "tl.cnv_copy_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos bool': (ValueError, 'tl.cnv_states: chr_pos start True is not an integer'),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_copy_states: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_copy_states: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_copy_states: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_copy_states: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_copy_states: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_copy_states: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_copy_states: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_copy_states: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_copy_states: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_copy_states: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_copy_states: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_copy_states: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_copy_states: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_copy_states: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_copy_states: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_copy_states: switch_prob='x' must be a number"),
        'switch_prob=5e-324': (ValueError, LOG_OF_ZERO),
        'switch_prob=1e-323, K = 8': (ValueError, 'tl.cnv_copy_states: switch_prob=1e-323 is too close to 0 or 1 for float64'),
        'switch_prob=1e-323, K = 6': (ValueError, 'tl.cnv_copy_states: switch_prob=1e-323 is too close to 0 or 1 for float64'),
        'switch_prob=1e-323, K = 3, then sigma': (ValueError, 'tl.cnv_copy_states: sigma=0 must be finite and > 0'),
        'switch_prob=1e-323, K = 2, then sigma': (ValueError, 'tl.cnv_copy_states: sigma=0 must be finite and > 0'),
        'levels with amplitude': (ValueError, 'tl.cnv_copy_states: levels and amplitude are both given; amplitude only spaces the default levels'),
        'levels not a sequence': (ValueError, 'tl.cnv_copy_states: levels=5 must be a sequence of numbers'),
        'levels string': (ValueError, "tl.cnv_copy_states: levels='ab' must be a sequence of numbers"),
        'levels none': (ValueError, 'tl.cnv_copy_states: levels=(0.0, None) must be a sequence of numbers'),
        'levels of one': (ValueError, 'tl.cnv_copy_states: levels has 1 states; the chain takes 2 to 8'),
        'levels of nine': (ValueError, 'tl.cnv_copy_states: levels has 9 states; the chain takes 2 to 8'),
        'levels nan': (ValueError, 'tl.cnv_copy_states: levels=[-0.3, 0.0, nan] must be finite'),
        'levels inf': (ValueError, 'tl.cnv_copy_states: levels=[-0.3, 0.0, inf] must be finite'),
        'levels descend': (ValueError, 'tl.cnv_copy_states: levels=[0.0, 0.5, 0.3] must ascend strictly'),
        'levels repeat': (ValueError, 'tl.cnv_copy_states: levels=[0.0, 0.3, 0.3] must ascend strictly'),
        'levels two zeros': (ValueError, 'tl.cnv_copy_states: levels=[-0.0, 0.0, 0.3] must ascend strictly'),
        'levels without 0': (ValueError, 'tl.cnv_copy_states: levels=[0.1, 0.2, 0.3] must hold exactly one 0.0, the neutral state'),
    },
    'cnv_copy_posteriors': {
        'missing obsm key': (KeyError, 'tl.cnv_copy_posteriors: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_copy_posteriors: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_copy_posteriors: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_copy_posteriors: empty matrix of shape (4, 0)'),
        'W above the cap, K = 6': (ValueError, "tl.cnv_copy_posteriors: 2926 windows; the kernel keeps a cell's windows and the forward variables of K = 6 states in LDS and takes at most 2925"),
        'W above the cap, K = 8': (ValueError, "tl.cnv_copy_posteriors: 2276 windows; the kernel keeps a cell's windows and the forward variables of K = 8 states in LDS and takes at most 2275"),
        'W above the cap, K = 2': (ValueError, "tl.cnv_copy_posteriors: 6827 windows; the kernel keeps a cell's windows and the forward variables of K = 2 states in LDS and takes at most 6826"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos bool': (ValueError, 'tl.cnv_states: chr_pos start True is not an integer'),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_copy_posteriors: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_copy_posteriors: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_copy_posteriors: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_copy_posteriors: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_copy_posteriors: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_copy_posteriors: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_copy_posteriors: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_copy_posteriors: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_copy_posteriors: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_copy_posteriors: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_copy_posteriors: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_copy_posteriors: switch_prob='x' must be a number"),
        'switch_prob=1e-320': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=1e-320 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 8': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=1e-17 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 6': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=1e-17 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 3, then sigma': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'switch_prob=1e-17, K = 2, then sigma': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'switch_prob=2e-16, K = 8, then sigma': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'levels with amplitude': (ValueError, 'tl.cnv_copy_posteriors: levels and amplitude are both given; amplitude only spaces the default levels'),
        'levels not a sequence': (ValueError, 'tl.cnv_copy_posteriors: levels=5 must be a sequence of numbers'),
        'levels string': (ValueError, "tl.cnv_copy_posteriors: levels='ab' must be a sequence of numbers"),
        'levels none': (ValueError, 'tl.cnv_copy_posteriors: levels=(0.0, None) must be a sequence of numbers'),
        'levels of one': (ValueError, 'tl.cnv_copy_posteriors: levels has 1 states; the chain takes 2 to 8'),
        'levels of nine': (ValueError, 'tl.cnv_copy_posteriors: levels has 9 states; the chain takes 2 to 8'),
        'levels nan': (ValueError, 'tl.cnv_copy_posteriors: levels=[-0.3, 0.0, nan] must be finite'),
        'levels inf': (ValueError, 'tl.cnv_copy_posteriors: levels=[-0.3, 0.0, inf] must be finite'),
        'levels descend': (ValueError, 'tl.cnv_copy_posteriors: levels=[0.0, 0.5, 0.3] must ascend strictly'),
        'levels repeat': (ValueError, 'tl.cnv_copy_posteriors: levels=[0.0, 0.3, 0.3] must ascend strictly'),
        'levels two zeros': (ValueError, 'tl.cnv_copy_posteriors: levels=[-0.0, 0.0, 0.3] must ascend strictly'),
        'levels without 0': (ValueError, 'tl.cnv_copy_posteriors: levels=[0.1, 0.2, 0.3] must hold exactly one 0.0, the neutral state'),
        'stored levels without 0': (ValueError, 'tl.cnv_copy_posteriors: levels=[0.1, 0.2] must hold exactly one 0.0, the neutral state'),
        'stored sigma': (ValueError, 'tl.cnv_copy_posteriors: sigma=-1.0 must be finite and > 0'),
        'stored switch_prob': (ValueError, 'tl.cnv_copy_posteriors: switch_prob=2.0 must lie in (0, 1)'),
        'stored K = 8 above its cap': (ValueError, "tl.cnv_copy_posteriors: 2276 windows; the kernel keeps a cell's windows and the forward variables of K = 8 states in LDS and takes at most 2275"),
    },
    'cnv_copy_states_fit': {
        'missing obsm key': (KeyError, 'tl.cnv_copy_states_fit: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing chr_pos': (KeyError, "tl.cnv_copy_states_fit: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D X': (ValueError, 'tl.cnv_copy_states_fit: X must be 2-D'),
        'empty shape': (ValueError, 'tl.cnv_copy_states_fit: empty matrix of shape (4, 0)'),
        'W above the cap, K = 6': (ValueError, "tl.cnv_copy_states_fit: 2924 windows; the kernel keeps a cell's windows, the forward variables of K = 6 states and 13 sums per chromosome (163840 bytes) in LDS and takes at most 2923"),
        'W above the cap, K = 8': (ValueError, "tl.cnv_copy_states_fit: 2274 windows; the kernel keeps a cell's windows, the forward variables of K = 8 states and 17 sums per chromosome (163840 bytes) in LDS and takes at most 2273"),
        'W above the cap, K = 2': (ValueError, "tl.cnv_copy_states_fit: 6826 windows; the kernel keeps a cell's windows, the forward variables of K = 2 states and 5 sums per chromosome (163840 bytes) in LDS and takes at most 6825"),
        'W above the cap of 23 chromosomes': (ValueError, "tl.cnv_copy_states_fit: 2884 windows in 23 chromosomes; the kernel keeps a cell's windows, the forward variables of K = 6 states and 13 sums per chromosome in 163840 bytes of LDS and takes at most 2883 windows"),
        'W above the cap of 23 chromosomes, K = 8': (ValueError, "tl.cnv_copy_states_fit: 2233 windows in 23 chromosomes; the kernel keeps a cell's windows, the forward variables of K = 8 states and 17 sums per chromosome in 163840 bytes of LDS and takes at most 2232 windows"),
        '2000 chromosomes fill the LDS, K = 8': (ValueError, "tl.cnv_copy_states_fit: 2000 windows in 2000 chromosomes; the kernel keeps a cell's windows, the forward variables of K = 8 states and 17 sums per chromosome in 163840 bytes of LDS and takes at most 0 windows"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos negative': (ValueError, 'tl.cnv_states: chr_pos start -1 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos bool': (ValueError, 'tl.cnv_states: chr_pos start True is not an integer'),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'amplitude=0': (ValueError, 'tl.cnv_copy_states_fit: amplitude=0 must be finite and > 0'),
        'amplitude=-1': (ValueError, 'tl.cnv_copy_states_fit: amplitude=-1 must be finite and > 0'),
        'amplitude=nan': (ValueError, 'tl.cnv_copy_states_fit: amplitude=nan must be finite and > 0'),
        'amplitude=inf': (ValueError, 'tl.cnv_copy_states_fit: amplitude=inf must be finite and > 0'),
        'amplitude=True': (ValueError, 'tl.cnv_copy_states_fit: amplitude=True must be finite and > 0'),
        "amplitude='x'": (ValueError, "tl.cnv_copy_states_fit: amplitude='x' must be a number"),
        'sigma=0': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'sigma=-1': (ValueError, 'tl.cnv_copy_states_fit: sigma=-1 must be finite and > 0'),
        'sigma=nan': (ValueError, 'tl.cnv_copy_states_fit: sigma=nan must be finite and > 0'),
        'sigma=inf': (ValueError, 'tl.cnv_copy_states_fit: sigma=inf must be finite and > 0'),
        'sigma=True': (ValueError, 'tl.cnv_copy_states_fit: sigma=True must be finite and > 0'),
        "sigma='x'": (ValueError, "tl.cnv_copy_states_fit: sigma='x' must be a number"),
        'switch_prob=0': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=0 must lie in (0, 1)'),
        'switch_prob=1': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=1 must lie in (0, 1)'),
        'switch_prob=True': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=True must lie in (0, 1)'),
        "switch_prob='x'": (ValueError, "tl.cnv_copy_states_fit: switch_prob='x' must be a number"),
        'switch_prob=1e-320': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=1e-320 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 8': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=1e-17 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 6': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=1e-17 is too close to 0 or 1 for float64'),
        'switch_prob=1e-17, K = 3, then sigma': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'switch_prob=1e-17, K = 2, then sigma': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'switch_prob=2e-16, K = 8, then sigma': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'steps not a sequence': (ValueError, 'tl.cnv_copy_states_fit: steps=5 must be a sequence of integers'),
        'steps string': (ValueError, "tl.cnv_copy_states_fit: steps='ab' must be integers"),
        'steps fraction': (ValueError, 'tl.cnv_copy_states_fit: steps=(0, 1.5) must be integers'),
        'steps bool': (ValueError, 'tl.cnv_copy_states_fit: steps=(0, True) must be integers'),
        'steps none': (ValueError, 'tl.cnv_copy_states_fit: steps=(0, None) must be integers'),
        'steps of one': (ValueError, 'tl.cnv_copy_states_fit: steps has 1 states; the chain takes 2 to 8'),
        'steps of nine': (ValueError, 'tl.cnv_copy_states_fit: steps has 9 states; the chain takes 2 to 8'),
        'steps descend': (ValueError, 'tl.cnv_copy_states_fit: steps=[0, 2, 1] must ascend strictly'),
        'steps repeat': (ValueError, 'tl.cnv_copy_states_fit: steps=[0, 1, 1] must ascend strictly'),
        'steps without 0': (ValueError, 'tl.cnv_copy_states_fit: steps=[1, 2, 3] must hold 0, the neutral state'),
        'fit unknown': (ValueError, "tl.cnv_copy_states_fit: fit=('nope',) must be a non-empty subset of ('amplitude', 'sigma', 'switch_prob')"),
        'fit not a sequence': (ValueError, 'tl.cnv_copy_states_fit: fit=3 must be a sequence of parameter names'),
        'fit empty': (ValueError, "tl.cnv_copy_states_fit: fit=() must be a non-empty subset of ('amplitude', 'sigma', 'switch_prob')"),
        'max_iter=0': (ValueError, 'tl.cnv_copy_states_fit: max_iter=0 must be an int >= 1'),
        'max_iter=True': (ValueError, 'tl.cnv_copy_states_fit: max_iter=True must be an int >= 1'),
        'max_iter=2.0': (ValueError, 'tl.cnv_copy_states_fit: max_iter=2.0 must be an int >= 1'),
        "tol='x'": (ValueError, "tl.cnv_copy_states_fit: tol='x' must be a number"),
        'tol=-1': (ValueError, 'tl.cnv_copy_states_fit: tol=-1 must be finite and >= 0'),
        'tol=nan': (ValueError, 'tl.cnv_copy_states_fit: tol=nan must be finite and >= 0'),
        'tol=True': (ValueError, 'tl.cnv_copy_states_fit: tol=True must be finite and >= 0'),
    },
    'cnv_copy_states_filter': {
        'missing calls': (KeyError, 'tl.cnv_copy_states_filter: X_cnv_copy_states not found in adata.obsm. Did you run `tl.cnv_states`?'),
        'missing posteriors': (KeyError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral not found in adata.obsm. Did you run `tl.cnv_posteriors`?'),
        'missing cnv': (KeyError, "tl.cnv_copy_states_filter: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        'other keys': (KeyError, 'tl.cnv_copy_states_filter: X_a not found in adata.obsm. Did you run `tl.cnv_states`?'),
        'other posterior key': (KeyError, 'tl.cnv_copy_states_filter: X_b_neutral not found in adata.obsm. Did you run `tl.cnv_posteriors`?'),
        'other cnv key': (KeyError, "tl.cnv_copy_states_filter: chr_pos not found in adata.uns['c']. Did you run `tl.infercnv`?"),
        '1-D calls': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_states must be 2-D'),
        'a list of calls': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_states must be 2-D'),
        'int32 calls': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_states must be int8 (-1 loss, 0 neutral, +1 gain), not int32'),
        'posteriors of another shape': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral has shape (4, 9), X_cnv_copy_states has (4, 10)'),
        'float32 posteriors': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral must be float64, not float32'),
        'empty matrix': (ValueError, 'tl.cnv_copy_states_filter: empty matrix of shape (0, 10)'),
        'W above the cap': (ValueError, "tl.cnv_copy_states_filter: 4194305 windows; a run's int64 sum takes at most 4194304"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos fraction': (ValueError, 'tl.cnv_states: chr_pos start 2.5 is not an integer'),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        "max_p_normal='x'": (ValueError, "tl.cnv_copy_states_filter: max_p_normal='x' must be a number in [0, 1]"),
        'max_p_normal=None': (ValueError, 'tl.cnv_copy_states_filter: max_p_normal=None must be a number in [0, 1]'),
        'max_p_normal=-0.1': (ValueError, 'tl.cnv_copy_states_filter: max_p_normal=-0.1 must lie in [0, 1]'),
        'max_p_normal=1.5': (ValueError, 'tl.cnv_copy_states_filter: max_p_normal=1.5 must lie in [0, 1]'),
        'max_p_normal=nan': (ValueError, 'tl.cnv_copy_states_filter: max_p_normal=nan must lie in [0, 1]'),
        'max_p_normal=True': (ValueError, 'tl.cnv_copy_states_filter: max_p_normal=True must lie in [0, 1]'),
    },
}

ORDER = {
    'cnv_copy_states': {
        'keys before shape': (KeyError, 'tl.cnv_copy_states: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'cap before chr_pos': (ValueError, "tl.cnv_copy_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
        'chr_pos before amplitude': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'amplitude before sigma': (ValueError, 'tl.cnv_copy_states: amplitude=0 must be finite and > 0'),
        'sigma before switch_prob': (ValueError, 'tl.cnv_copy_states: sigma=0 must be finite and > 0'),
        'sigma before switch_prob, K = 8': (ValueError, 'tl.cnv_copy_states: sigma=0 must be finite and > 0'),
        'levels with amplitude before levels': (ValueError, 'tl.cnv_copy_states: levels and amplitude are both given; amplitude only spaces the default levels'),
        'levels before keys': (ValueError, 'tl.cnv_copy_states: levels=[0.1, 0.2] must hold exactly one 0.0, the neutral state'),
        'the cap is that of the given K': (ValueError, "tl.cnv_copy_states: 16385 windows; the kernel keeps a cell's windows in LDS and takes at most 16384"),
    },
    'cnv_copy_posteriors': {
        'keys before shape': (KeyError, 'tl.cnv_copy_posteriors: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'cap before chr_pos': (ValueError, "tl.cnv_copy_posteriors: 16385 windows; the kernel keeps a cell's windows and the forward variables of K = 6 states in LDS and takes at most 2925"),
        'chr_pos before amplitude': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'amplitude before sigma': (ValueError, 'tl.cnv_copy_posteriors: amplitude=0 must be finite and > 0'),
        'sigma before switch_prob': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'sigma before switch_prob, K = 8': (ValueError, 'tl.cnv_copy_posteriors: sigma=0 must be finite and > 0'),
        'levels with amplitude before levels': (ValueError, 'tl.cnv_copy_posteriors: levels and amplitude are both given; amplitude only spaces the default levels'),
        'levels before keys': (ValueError, 'tl.cnv_copy_posteriors: levels=[0.1, 0.2] must hold exactly one 0.0, the neutral state'),
        'the cap is that of the given K': (ValueError, "tl.cnv_copy_posteriors: 2276 windows; the kernel keeps a cell's windows and the forward variables of K = 8 states in LDS and takes at most 2275"),
    },
    'cnv_copy_states_fit': {
        'keys before shape': (KeyError, 'tl.cnv_copy_states_fit: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'cap before chr_pos': (ValueError, "tl.cnv_copy_states_fit: 16385 windows; the kernel keeps a cell's windows, the forward variables of K = 6 states and 13 sums per chromosome (163840 bytes) in LDS and takes at most 2923"),
        'chr_pos before amplitude': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'amplitude before sigma': (ValueError, 'tl.cnv_copy_states_fit: amplitude=0 must be finite and > 0'),
        'sigma before switch_prob': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'sigma before switch_prob, K = 8': (ValueError, 'tl.cnv_copy_states_fit: sigma=0 must be finite and > 0'),
        'steps before keys': (ValueError, 'tl.cnv_copy_states_fit: steps=[1, 2] must hold 0, the neutral state'),
        'switch_prob before fit': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=0 must lie in (0, 1)'),
        'switch_prob before the cap of the chromosomes': (ValueError, 'tl.cnv_copy_states_fit: switch_prob=1e-17 is too close to 0 or 1 for float64'),
        'the cap of the chromosomes before fit': (ValueError, "tl.cnv_copy_states_fit: 2884 windows in 23 chromosomes; the kernel keeps a cell's windows, the forward variables of K = 6 states and 13 sums per chromosome in 163840 bytes of LDS and takes at most 2883 windows"),
        'fit before max_iter': (ValueError, "tl.cnv_copy_states_fit: fit=() must be a non-empty subset of ('amplitude', 'sigma', 'switch_prob')"),
        'max_iter before tol': (ValueError, 'tl.cnv_copy_states_fit: max_iter=0 must be an int >= 1'),
    },
    'cnv_copy_states_filter': {
        'calls before posteriors': (KeyError, 'tl.cnv_copy_states_filter: X_cnv_copy_states not found in adata.obsm. Did you run `tl.cnv_states`?'),
        'posteriors before chr_pos': (KeyError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral not found in adata.obsm. Did you run `tl.cnv_posteriors`?'),
        'chr_pos before dtype': (KeyError, "tl.cnv_copy_states_filter: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        'dtype of the calls before the shape of the posteriors': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_states must be int8 (-1 loss, 0 neutral, +1 gain), not float64'),
        'shape before dtype of the posteriors': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral has shape (4, 9), X_cnv_copy_states has (4, 10)'),
        'dtype of the posteriors before empty': (ValueError, 'tl.cnv_copy_states_filter: X_cnv_copy_posterior_neutral must be float64, not float32'),
        'cap before chr_pos': (ValueError, "tl.cnv_copy_states_filter: 4194305 windows; a run's int64 sum takes at most 4194304"),
        'chr_pos before max_p_normal': (ValueError, 'tl.cnv_states: chr_pos is empty'),
    },
}


def _raised(call):
    """(the exception's type, its first argument) of a call that must raise."""
    with pytest.raises(Exception) as info:
        call()
    return type(info.value), info.value.args[0]


@pytest.mark.parametrize("fn", CHAIN)
def test_every_bad_input_keeps_its_exception_and_its_whole_message(fn):
    import infercnvpy_amd as cnv

    cases = _chain_cases(fn)
    assert [cid for cid, _, _ in cases] == list(EXPECTED[fn])
    for cid, make, kw in cases:
        assert _raised(lambda: getattr(cnv.tl, fn)(make(), **kw)) == EXPECTED[fn][cid], (fn, cid)


@pytest.mark.parametrize("fn", CHAIN)
def test_the_first_fault_in_the_order_of_the_checks_is_the_one_reported(fn):
    import infercnvpy_amd as cnv

    cases = _order_cases(fn)
    assert [cid for cid, _, _ in cases] == list(ORDER[fn])
    for cid, make, kw in cases:
        assert _raised(lambda: getattr(cnv.tl, fn)(make(), **kw)) == ORDER[fn][cid], (fn, cid)


# ---- tl.cnv_copy_states_filter ---------------------------------------------------------------------------------------------------
def _filter_adata(states=None, post=None, chr_pos=None, drop=()):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((4, 3), dtype=np.float32))
    ad.obsm["X_cnv_copy_states"] = np.zeros((4, 10), dtype=np.int8) if states is None else states
    ad.obsm["X_cnv_copy_posterior_neutral"] = np.ones((4, 10)) if post is None else post
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    for where, key in drop:
        del getattr(ad, where)[key]
    return ad


def _flat(dtype, shape):
    """An array of ``shape`` that takes one element of memory."""
    return np.broadcast_to(np.zeros(1, dtype=dtype), shape)


def _filter_cases():
    fa = _filter_adata
    out = [
        ("missing calls", lambda: fa(drop=[("obsm", "X_cnv_copy_states")]), {}),
        ("missing posteriors", lambda: fa(drop=[("obsm", "X_cnv_copy_posterior_neutral")]), {}),
        ("missing cnv", lambda: fa(drop=[("uns", "cnv")]), {}),
        ("other keys", fa, {"use_rep": "a", "posterior_key": "b", "cnv_key": "c"}),
        ("other posterior key", fa, {"posterior_key": "b"}),
        ("other cnv key", fa, {"cnv_key": "c"}),
        ("1-D calls", lambda: fa(states=np.zeros(4, dtype=np.int8)), {}),
        ("a list of calls", lambda: fa(states=[[0] * 10] * 4), {}),
        ("int32 calls", lambda: fa(states=np.zeros((4, 10), dtype=np.int32)), {}),
        ("posteriors of another shape", lambda: fa(post=np.ones((4, 9))), {}),
        ("float32 posteriors", lambda: fa(post=np.ones((4, 10), dtype=np.float32)), {}),
        ("empty matrix", lambda: fa(states=np.zeros((0, 10), dtype=np.int8), post=np.ones((0, 10))), {}),
        ("W above the cap", lambda: fa(states=_flat(np.int8, (1, FILTER_CAP + 1)), post=_flat(np.float64, (1, FILTER_CAP + 1))), {}),
    ]
    for cid, chr_pos in [
        ("chr_pos outside", {"chr1": 0, "chr2": 10}), ("chr_pos same window", {"chr1": 0, "chr2": 4, "chr3": 4}),
        ("chr_pos not at 0", {"chr1": 1, "chr2": 4}), ("chr_pos fraction", {"chr1": 0, "chr2": 2.5}),
        ("chr_pos empty", {}), ("chr_pos list", [0, 4]),
    ]:
        out.append((cid, (lambda c=chr_pos: fa(chr_pos=c)), {}))
    for v in ("x", None, -0.1, 1.5, float("nan"), True):
        out.append((f"max_p_normal={v!r}", fa, {"max_p_normal": v}))
    return out


def _filter_order_cases():
    fa = _filter_adata
    return [
        ("calls before posteriors", lambda: fa(drop=[("obsm", "X_cnv_copy_states"), ("obsm", "X_cnv_copy_posterior_neutral")]), {}),
        ("posteriors before chr_pos", lambda: fa(drop=[("obsm", "X_cnv_copy_posterior_neutral"), ("uns", "cnv")]), {}),
        ("chr_pos before dtype", lambda: fa(states=np.zeros((4, 10)), drop=[("uns", "cnv")]), {}),
        ("dtype of the calls before the shape of the posteriors", lambda: fa(states=np.zeros((4, 10)), post=np.ones((4, 9))), {}),
        ("shape before dtype of the posteriors", lambda: fa(post=np.ones((4, 9), dtype=np.float32)), {}),
        ("dtype of the posteriors before empty", lambda: fa(states=np.zeros((0, 10), dtype=np.int8), post=np.ones((0, 10), dtype=np.float32)), {}),
        ("cap before chr_pos", lambda: fa(states=_flat(np.int8, (1, FILTER_CAP + 1)), post=_flat(np.float64, (1, FILTER_CAP + 1)), chr_pos={}), {}),
        ("chr_pos before max_p_normal", lambda: fa(chr_pos={}), {"max_p_normal": 2}),
    ]


def test_every_bad_input_of_the_filter_keeps_its_exception_and_its_whole_message():
    import infercnvpy_amd as cnv

    for cases, table in ((_filter_cases(), EXPECTED["cnv_copy_states_filter"]), (_filter_order_cases(), ORDER["cnv_copy_states_filter"])):
        assert [cid for cid, _, _ in cases] == list(table)
        for cid, make, kw in cases:
            assert _raised(lambda: cnv.tl.cnv_copy_states_filter(make(), **kw)) == table[cid], cid


# ---- the four entry points -----------------------------------------------------------------------------------------------------
ONE = ctypes.c_void_p(16)  # never dereferenced: every call below fails in the argument checks
SIX = [0.3 * s for s in (-2, -1, 0, 1, 2, 3)]
CHAIN_ENTRIES = ("icv_copy_states_viterbi", "icv_copy_posterior_chains", "icv_copy_posterior_stats")


def _matrix(n_cols, n_rows=0, complete=True, fmt=None, dtype=None, ld=None):
    from infercnvpy_amd import _lib

    fmt = _lib.ICV_CSR if fmt is None else fmt
    m = _lib.Matrix(format=fmt, dtype=_lib.ICV_F64 if dtype is None else dtype, n_rows=n_rows, n_cols=n_cols,
                    ld=n_cols if ld is None else ld)
    if complete:
        m.indptr, m.values = 16, 16
    return m


def _chain_entry(entry, mat, n_chr=1, chr_start=ONE, levels=SIX, n_levels=None, neutral=2, h=50.0, a=None, b=None,
                 outputs=None):
    """(status, message) of one call of a chain entry; a, b: stay, sw of the Viterbi entry and ps, pw of the others."""
    from infercnvpy_amd import _lib

    lib = _lib.load()
    viterbi = entry == "icv_copy_states_viterbi"
    if a is None:
        a = math.log(0.999) if viterbi else 0.999
    if b is None:
        b = math.log(0.0002) if viterbi else 0.0002
    if outputs is None:
        outputs = {"icv_copy_states_viterbi": (ONE, ONE, ONE), "icv_copy_posterior_chains": (ONE, None),
                   "icv_copy_posterior_stats": (ONE,)}[entry]
    mu = None if levels is None else (ctypes.c_double * max(len(levels), 1))(*levels)
    k = n_levels if n_levels is not None else 6 if levels is None else len(levels)
    rc = getattr(lib, entry)(None if mat is None else ctypes.byref(mat), chr_start, n_chr, mu, k, neutral, h, a, b,
                             *outputs, None)
    return rc, lib.icv_last_error().decode()


def _entry_cases(entry):
    """(id, keywords of _chain_entry) of every refusal of a chain entry."""
    from infercnvpy_amd import _lib

    viterbi = entry == "icv_copy_states_viterbi"
    stats = entry == "icv_copy_posterior_stats"
    n_out = {"icv_copy_states_viterbi": 3, "icv_copy_posterior_chains": 1, "icv_copy_posterior_stats": 1}[entry]
    m = _matrix(8)
    inf, nan = math.inf, math.nan

    def cap(k, n_chr=1):
        return 16384 if viterbi else stats_cap(k, n_chr) if stats else chain_cap(k)

    out = [("no matrix", dict(mat=None)), ("no chr_start", dict(mat=m, chr_start=None)), ("no levels", dict(mat=m, levels=None)),
           ("n_chr = 0", dict(mat=m, n_chr=0)), ("negative rows", dict(mat=_matrix(8, n_rows=-1))),
           ("a format that is none", dict(mat=_matrix(8, fmt=7))), ("a dtype that is none", dict(mat=_matrix(8, dtype=7)))]
    for i in range(n_out):
        optional = (ONE,) if entry == "icv_copy_posterior_chains" else ()  # (the planes may be null)
        out.append((f"no output {i}", dict(mat=m, outputs=tuple(None if j == i else ONE for j in range(n_out)) + optional)))
    out += [("n_cols = 0", dict(mat=_matrix(0))),
            ("n_cols above the cap, K = 6", dict(mat=_matrix(cap(6) + 1))),
            ("n_cols above the cap, K = 2", dict(mat=_matrix(cap(2) + 1), levels=[0.0, 0.3], neutral=0)),
            ("n_cols above the cap, K = 8", dict(mat=_matrix(cap(8) + 1), levels=EIGHT, neutral=3)),
            # an n_levels outside [2, 8]: the cap of the message is that of the clamped K
            ("n_cols above the cap, n_levels = 1", dict(mat=_matrix(cap(2) + 1), levels=[0.0], neutral=0)),
            ("n_cols above the cap, n_levels = -3", dict(mat=_matrix(cap(2) + 1), n_levels=-3)),
            ("n_cols above the cap, n_levels = 9", dict(mat=_matrix(cap(8) + 1), levels=[0.1 * s for s in range(9)], neutral=0))]
    if stats:
        out += [("n_cols above the cap of 23 chromosomes", dict(mat=_matrix(cap(6, 23) + 1), n_chr=23)),
                ("2000 chromosomes fill the LDS, n_levels = 9", dict(mat=_matrix(2000), n_chr=2000, n_levels=9))]
    out += [("more chromosomes than windows", dict(mat=m, n_chr=9)),
            ("n_levels = 1", dict(mat=m, levels=[0.0], neutral=0)), ("n_levels = 0", dict(mat=m, n_levels=0)),
            ("n_levels = 9", dict(mat=m, levels=[0.1 * s for s in range(9)], neutral=0)),
            ("neutral = -1", dict(mat=m, neutral=-1)), ("neutral = 6", dict(mat=m, neutral=6)),
            ("levels inf", dict(mat=m, levels=[-0.3, 0.0, inf], neutral=1)),
            ("levels nan", dict(mat=m, levels=[-0.3, nan, 0.3], neutral=1)),
            ("levels repeat", dict(mat=m, levels=[-0.3, 0.0, 0.0], neutral=1)),
            ("levels descend", dict(mat=m, levels=[0.3, 0.0, -0.3], neutral=1)),
            ("levels[neutral] is not 0", dict(mat=m, neutral=1)),
            ("h = 0", dict(mat=m, h=0.0)), ("h = -1", dict(mat=m, h=-1.0)), ("h = inf", dict(mat=m, h=inf)),
            ("h = nan", dict(mat=m, h=nan))]
    if viterbi:
        out += [("stay = -inf", dict(mat=m, a=-inf)), ("stay = nan", dict(mat=m, a=nan)), ("sw = -inf", dict(mat=m, b=-inf)),
                ("sw = nan", dict(mat=m, b=nan))]
    else:
        out += [("ps = 0", dict(mat=m, a=0.0)), ("ps = 1", dict(mat=m, a=1.0)), ("ps = nan", dict(mat=m, a=nan)),
                ("pw = 0", dict(mat=m, b=0.0)), ("pw subnormal", dict(mat=m, b=1e-320)), ("pw = 1", dict(mat=m, b=1.0)),
                ("pw = -0.1", dict(mat=m, b=-0.1)), ("pw = nan", dict(mat=m, b=nan))]
    out += [("incomplete CSR", dict(mat=_matrix(8, complete=False))),
            ("incomplete dense", dict(mat=_matrix(8, complete=False, fmt=_lib.ICV_DENSE))),
            ("dense with ld below n_cols", dict(mat=_matrix(8, fmt=_lib.ICV_DENSE, ld=7))),
            ("2^31 rows", dict(mat=_matrix(8, n_rows=1 << 31))),
            # two faults: the pointers, the window range, the chromosomes, the model (in its own order), the matrix, the rows
            ("order: pointers before n_cols", dict(mat=_matrix(0), n_chr=0, neutral=9)),
            ("order: n_cols before chromosomes", dict(mat=_matrix(0), n_chr=9, neutral=9)),
            ("order: chromosomes before the model", dict(mat=m, n_chr=9, neutral=9)),
            ("order: n_levels before neutral", dict(mat=m, levels=[0.0], neutral=5)),
            ("order: neutral before the levels", dict(mat=m, levels=[0.3, nan, 0.0], neutral=3)),
            ("order: finite before ascending", dict(mat=m, levels=[0.3, nan, 0.0], neutral=2)),
            ("order: ascending before the neutral level", dict(mat=m, levels=[0.3, 0.2, 0.1], neutral=2)),
            ("order: the neutral level before h", dict(mat=m, neutral=1, h=0.0)),
            ("order: h before the transition scalars", dict(mat=m, h=0.0, a=nan)),
            ("order: the model before the matrix", dict(mat=_matrix(8, complete=False), neutral=9)),
            ("order: the matrix before the rows", dict(mat=_matrix(8, n_rows=1 << 31, complete=False)))]
    return out


ENTRY = {
    'icv_copy_states_viterbi': {
        'no matrix': (INVALID, 'bad copy_states_viterbi arguments'),
        'no chr_start': (INVALID, 'bad copy_states_viterbi arguments'),
        'no levels': (INVALID, 'bad copy_states_viterbi arguments'),
        'n_chr = 0': (INVALID, 'bad copy_states_viterbi arguments'),
        'negative rows': (INVALID, 'bad copy_states_viterbi arguments'),
        'a format that is none': (INVALID, 'bad copy_states_viterbi arguments'),
        'a dtype that is none': (INVALID, 'bad copy_states_viterbi arguments'),
        'no output 0': (INVALID, 'bad copy_states_viterbi arguments'),
        'no output 1': (INVALID, 'bad copy_states_viterbi arguments'),
        'no output 2': (INVALID, 'bad copy_states_viterbi arguments'),
        'n_cols = 0': (INVALID, 'copy_states_viterbi: n_cols = 0 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, K = 6': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, K = 2': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, K = 8': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, n_levels = 1': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, n_levels = -3': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'n_cols above the cap, n_levels = 9': (INVALID, 'copy_states_viterbi: n_cols = 16385 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'more chromosomes than windows': (INVALID, 'copy_states_viterbi: more chromosomes than windows'),
        'n_levels = 1': (INVALID, 'copy_states_viterbi: n_levels must lie in [2, 8]'),
        'n_levels = 0': (INVALID, 'copy_states_viterbi: n_levels must lie in [2, 8]'),
        'n_levels = 9': (INVALID, 'copy_states_viterbi: n_levels must lie in [2, 8]'),
        'neutral = -1': (INVALID, 'copy_states_viterbi: neutral must be the index of a level'),
        'neutral = 6': (INVALID, 'copy_states_viterbi: neutral must be the index of a level'),
        'levels inf': (INVALID, 'copy_states_viterbi: the levels must be finite'),
        'levels nan': (INVALID, 'copy_states_viterbi: the levels must be finite'),
        'levels repeat': (INVALID, 'copy_states_viterbi: the levels must ascend strictly'),
        'levels descend': (INVALID, 'copy_states_viterbi: the levels must ascend strictly'),
        'levels[neutral] is not 0': (INVALID, 'copy_states_viterbi: levels[neutral] must be 0'),
        'h = 0': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'h = -1': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'h = inf': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'h = nan': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'stay = -inf': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'stay = nan': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'sw = -inf': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'sw = nan': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'incomplete CSR': (INVALID, 'copy_states_viterbi: incomplete matrix'),
        'incomplete dense': (INVALID, 'copy_states_viterbi: incomplete matrix'),
        'dense with ld below n_cols': (INVALID, 'copy_states_viterbi: incomplete matrix'),
        '2^31 rows': (UNSUPPORTED, 'copy_states_viterbi: more than 2^31 - 1 rows in one call'),
        'order: pointers before n_cols': (INVALID, 'bad copy_states_viterbi arguments'),
        'order: n_cols before chromosomes': (INVALID, 'copy_states_viterbi: n_cols = 0 must lie in [1, 16384] (10 bytes of LDS per window)'),
        'order: chromosomes before the model': (INVALID, 'copy_states_viterbi: more chromosomes than windows'),
        'order: n_levels before neutral': (INVALID, 'copy_states_viterbi: n_levels must lie in [2, 8]'),
        'order: neutral before the levels': (INVALID, 'copy_states_viterbi: neutral must be the index of a level'),
        'order: finite before ascending': (INVALID, 'copy_states_viterbi: the levels must be finite'),
        'order: ascending before the neutral level': (INVALID, 'copy_states_viterbi: the levels must ascend strictly'),
        'order: the neutral level before h': (INVALID, 'copy_states_viterbi: levels[neutral] must be 0'),
        'order: h before the transition scalars': (INVALID, 'copy_states_viterbi: h must be finite and > 0, stay and sw finite'),
        'order: the model before the matrix': (INVALID, 'copy_states_viterbi: neutral must be the index of a level'),
        'order: the matrix before the rows': (INVALID, 'copy_states_viterbi: incomplete matrix'),
    },
    'icv_copy_posterior_chains': {
        'no matrix': (INVALID, 'bad copy_posterior_chains arguments'),
        'no chr_start': (INVALID, 'bad copy_posterior_chains arguments'),
        'no levels': (INVALID, 'bad copy_posterior_chains arguments'),
        'n_chr = 0': (INVALID, 'bad copy_posterior_chains arguments'),
        'negative rows': (INVALID, 'bad copy_posterior_chains arguments'),
        'a format that is none': (INVALID, 'bad copy_posterior_chains arguments'),
        'a dtype that is none': (INVALID, 'bad copy_posterior_chains arguments'),
        'no output 0': (INVALID, 'bad copy_posterior_chains arguments'),
        'n_cols = 0': (INVALID, 'copy_posterior_chains: n_cols = 0 must lie in [1, 2925] (56 bytes of LDS per window with K = 6 states)'),
        'n_cols above the cap, K = 6': (INVALID, 'copy_posterior_chains: n_cols = 2926 must lie in [1, 2925] (56 bytes of LDS per window with K = 6 states)'),
        'n_cols above the cap, K = 2': (INVALID, 'copy_posterior_chains: n_cols = 6827 must lie in [1, 6826] (24 bytes of LDS per window with K = 2 states)'),
        'n_cols above the cap, K = 8': (INVALID, 'copy_posterior_chains: n_cols = 2276 must lie in [1, 2275] (72 bytes of LDS per window with K = 8 states)'),
        'n_cols above the cap, n_levels = 1': (INVALID, 'copy_posterior_chains: n_cols = 6827 must lie in [1, 6826] (24 bytes of LDS per window with K = 2 states)'),
        'n_cols above the cap, n_levels = -3': (INVALID, 'copy_posterior_chains: n_cols = 6827 must lie in [1, 6826] (24 bytes of LDS per window with K = 2 states)'),
        'n_cols above the cap, n_levels = 9': (INVALID, 'copy_posterior_chains: n_cols = 2276 must lie in [1, 2275] (72 bytes of LDS per window with K = 8 states)'),
        'more chromosomes than windows': (INVALID, 'copy_posterior_chains: more chromosomes than windows'),
        'n_levels = 1': (INVALID, 'copy_posterior_chains: n_levels must lie in [2, 8]'),
        'n_levels = 0': (INVALID, 'copy_posterior_chains: n_levels must lie in [2, 8]'),
        'n_levels = 9': (INVALID, 'copy_posterior_chains: n_levels must lie in [2, 8]'),
        'neutral = -1': (INVALID, 'copy_posterior_chains: neutral must be the index of a level'),
        'neutral = 6': (INVALID, 'copy_posterior_chains: neutral must be the index of a level'),
        'levels inf': (INVALID, 'copy_posterior_chains: the levels must be finite'),
        'levels nan': (INVALID, 'copy_posterior_chains: the levels must be finite'),
        'levels repeat': (INVALID, 'copy_posterior_chains: the levels must ascend strictly'),
        'levels descend': (INVALID, 'copy_posterior_chains: the levels must ascend strictly'),
        'levels[neutral] is not 0': (INVALID, 'copy_posterior_chains: levels[neutral] must be 0'),
        'h = 0': (INVALID, 'copy_posterior_chains: h must be finite and > 0, stay and sw finite'),
        'h = -1': (INVALID, 'copy_posterior_chains: h must be finite and > 0, stay and sw finite'),
        'h = inf': (INVALID, 'copy_posterior_chains: h must be finite and > 0, stay and sw finite'),
        'h = nan': (INVALID, 'copy_posterior_chains: h must be finite and > 0, stay and sw finite'),
        'ps = 0': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'ps = 1': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'ps = nan': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = 0': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw subnormal': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = 1': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = -0.1': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = nan': (INVALID, 'copy_posterior_chains: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'incomplete CSR': (INVALID, 'copy_posterior_chains: incomplete matrix'),
        'incomplete dense': (INVALID, 'copy_posterior_chains: incomplete matrix'),
        'dense with ld below n_cols': (INVALID, 'copy_posterior_chains: incomplete matrix'),
        '2^31 rows': (UNSUPPORTED, 'copy_posterior_chains: more than 2^31 - 1 rows in one call'),
        'order: pointers before n_cols': (INVALID, 'bad copy_posterior_chains arguments'),
        'order: n_cols before chromosomes': (INVALID, 'copy_posterior_chains: n_cols = 0 must lie in [1, 2925] (56 bytes of LDS per window with K = 6 states)'),
        'order: chromosomes before the model': (INVALID, 'copy_posterior_chains: more chromosomes than windows'),
        'order: n_levels before neutral': (INVALID, 'copy_posterior_chains: n_levels must lie in [2, 8]'),
        'order: neutral before the levels': (INVALID, 'copy_posterior_chains: neutral must be the index of a level'),
        'order: finite before ascending': (INVALID, 'copy_posterior_chains: the levels must be finite'),
        'order: ascending before the neutral level': (INVALID, 'copy_posterior_chains: the levels must ascend strictly'),
        'order: the neutral level before h': (INVALID, 'copy_posterior_chains: levels[neutral] must be 0'),
        'order: h before the transition scalars': (INVALID, 'copy_posterior_chains: h must be finite and > 0, stay and sw finite'),
        'order: the model before the matrix': (INVALID, 'copy_posterior_chains: neutral must be the index of a level'),
        'order: the matrix before the rows': (INVALID, 'copy_posterior_chains: incomplete matrix'),
    },
    'icv_copy_posterior_stats': {
        'no matrix': (INVALID, 'bad copy_posterior_stats arguments'),
        'no chr_start': (INVALID, 'bad copy_posterior_stats arguments'),
        'no levels': (INVALID, 'bad copy_posterior_stats arguments'),
        'n_chr = 0': (INVALID, 'bad copy_posterior_stats arguments'),
        'negative rows': (INVALID, 'bad copy_posterior_stats arguments'),
        'a format that is none': (INVALID, 'bad copy_posterior_stats arguments'),
        'a dtype that is none': (INVALID, 'bad copy_posterior_stats arguments'),
        'no output 0': (INVALID, 'bad copy_posterior_stats arguments'),
        'n_cols = 0': (INVALID, 'copy_posterior_stats: n_cols = 0 must lie in [1, 2923] (56 bytes of LDS per window with K = 6 states, beside 104 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, K = 6': (INVALID, 'copy_posterior_stats: n_cols = 2924 must lie in [1, 2923] (56 bytes of LDS per window with K = 6 states, beside 104 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, K = 2': (INVALID, 'copy_posterior_stats: n_cols = 6826 must lie in [1, 6825] (24 bytes of LDS per window with K = 2 states, beside 40 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, K = 8': (INVALID, 'copy_posterior_stats: n_cols = 2274 must lie in [1, 2273] (72 bytes of LDS per window with K = 8 states, beside 136 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, n_levels = 1': (INVALID, 'copy_posterior_stats: n_cols = 6826 must lie in [1, 6825] (24 bytes of LDS per window with K = 2 states, beside 40 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, n_levels = -3': (INVALID, 'copy_posterior_stats: n_cols = 6826 must lie in [1, 6825] (24 bytes of LDS per window with K = 2 states, beside 40 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap, n_levels = 9': (INVALID, 'copy_posterior_stats: n_cols = 2274 must lie in [1, 2273] (72 bytes of LDS per window with K = 8 states, beside 136 bytes for each of the 1 chromosomes, of 163840 bytes)'),
        'n_cols above the cap of 23 chromosomes': (INVALID, 'copy_posterior_stats: n_cols = 2884 must lie in [1, 2883] (56 bytes of LDS per window with K = 6 states, beside 104 bytes for each of the 23 chromosomes, of 163840 bytes)'),
        '2000 chromosomes fill the LDS, n_levels = 9': (INVALID, 'copy_posterior_stats: n_cols = 2000 must lie in [1, 0] (72 bytes of LDS per window with K = 8 states, beside 136 bytes for each of the 2000 chromosomes, of 163840 bytes)'),
        'more chromosomes than windows': (INVALID, 'copy_posterior_stats: more chromosomes than windows'),
        'n_levels = 1': (INVALID, 'copy_posterior_stats: n_levels must lie in [2, 8]'),
        'n_levels = 0': (INVALID, 'copy_posterior_stats: n_levels must lie in [2, 8]'),
        'n_levels = 9': (INVALID, 'copy_posterior_stats: n_levels must lie in [2, 8]'),
        'neutral = -1': (INVALID, 'copy_posterior_stats: neutral must be the index of a level'),
        'neutral = 6': (INVALID, 'copy_posterior_stats: neutral must be the index of a level'),
        'levels inf': (INVALID, 'copy_posterior_stats: the levels must be finite'),
        'levels nan': (INVALID, 'copy_posterior_stats: the levels must be finite'),
        'levels repeat': (INVALID, 'copy_posterior_stats: the levels must ascend strictly'),
        'levels descend': (INVALID, 'copy_posterior_stats: the levels must ascend strictly'),
        'levels[neutral] is not 0': (INVALID, 'copy_posterior_stats: levels[neutral] must be 0'),
        'h = 0': (INVALID, 'copy_posterior_stats: h must be finite and > 0, stay and sw finite'),
        'h = -1': (INVALID, 'copy_posterior_stats: h must be finite and > 0, stay and sw finite'),
        'h = inf': (INVALID, 'copy_posterior_stats: h must be finite and > 0, stay and sw finite'),
        'h = nan': (INVALID, 'copy_posterior_stats: h must be finite and > 0, stay and sw finite'),
        'ps = 0': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'ps = 1': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'ps = nan': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = 0': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw subnormal': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = 1': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = -0.1': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'pw = nan': (INVALID, 'copy_posterior_stats: ps = 1 - p and pw = p / (n_levels - 1) for a p in (0, 1): ps in (0, 1), pw a normal float64 in (0, 1)'),
        'incomplete CSR': (INVALID, 'copy_posterior_stats: incomplete matrix'),
        'incomplete dense': (INVALID, 'copy_posterior_stats: incomplete matrix'),
        'dense with ld below n_cols': (INVALID, 'copy_posterior_stats: incomplete matrix'),
        '2^31 rows': (UNSUPPORTED, 'copy_posterior_stats: more than 2^31 - 1 rows in one call'),
        'order: pointers before n_cols': (INVALID, 'bad copy_posterior_stats arguments'),
        'order: n_cols before chromosomes': (INVALID, 'copy_posterior_stats: n_cols = 0 must lie in [1, 2909] (56 bytes of LDS per window with K = 6 states, beside 104 bytes for each of the 9 chromosomes, of 163840 bytes)'),
        'order: chromosomes before the model': (INVALID, 'copy_posterior_stats: more chromosomes than windows'),
        'order: n_levels before neutral': (INVALID, 'copy_posterior_stats: n_levels must lie in [2, 8]'),
        'order: neutral before the levels': (INVALID, 'copy_posterior_stats: neutral must be the index of a level'),
        'order: finite before ascending': (INVALID, 'copy_posterior_stats: the levels must be finite'),
        'order: ascending before the neutral level': (INVALID, 'copy_posterior_stats: the levels must ascend strictly'),
        'order: the neutral level before h': (INVALID, 'copy_posterior_stats: levels[neutral] must be 0'),
        'order: h before the transition scalars': (INVALID, 'copy_posterior_stats: h must be finite and > 0, stay and sw finite'),
        'order: the model before the matrix': (INVALID, 'copy_posterior_stats: neutral must be the index of a level'),
        'order: the matrix before the rows': (INVALID, 'copy_posterior_stats: incomplete matrix'),
    },
    'icv_copy_states_filter': {
        'no pointer 0': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 1': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 2': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 3': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 4': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 5': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 6': (INVALID, 'bad copy_states_filter arguments'),
        'no pointer 7': (INVALID, 'bad copy_states_filter arguments'),
        'negative rows': (INVALID, 'bad copy_states_filter arguments'),
        'n_cols = 0': (INVALID, 'bad copy_states_filter arguments'),
        'n_chr = 0': (INVALID, 'bad copy_states_filter arguments'),
        'more chromosomes than windows': (INVALID, 'bad copy_states_filter arguments'),
        'max_p_normal = -0.1': (INVALID, 'bad copy_states_filter arguments'),
        'max_p_normal = 1.5': (INVALID, 'bad copy_states_filter arguments'),
        'max_p_normal = nan': (INVALID, 'bad copy_states_filter arguments'),
        'n_cols above the cap': (UNSUPPORTED, 'copy_states_filter: n_cols = 4194305 is above 4194304 (the int64 sum of a run)'),
        'order: the arguments before the cap': (INVALID, 'bad copy_states_filter arguments'),
    },
}


@pytest.mark.parametrize("entry", CHAIN_ENTRIES)
def test_every_refusal_of_a_chain_entry_keeps_its_status_and_its_whole_message(entry):
    from infercnvpy_amd import _lib

    assert _chain_entry(entry, _matrix(8))[0] == _lib.ICV_OK  # no rows: nothing runs
    cases = _entry_cases(entry)
    assert [cid for cid, _ in cases] == list(ENTRY[entry])
    for cid, kw in cases:
        assert _chain_entry(entry, **kw) == ENTRY[entry][cid], (entry, cid)


def _filter_entry(n_rows=4, n_cols=10, n_chr=2, thr=0.5, missing=None):
    from infercnvpy_amd import _lib

    lib = _lib.load()
    states, p, chr_start, filtered, sign, count, removed, bad = (None if i == missing else ONE for i in range(8))
    rc = lib.icv_copy_states_filter(states, p, n_rows, n_cols, chr_start, n_chr, thr, filtered, sign, count, removed, bad, None)
    return rc, lib.icv_last_error().decode()


def _filter_entry_cases():
    out = [(f"no pointer {i}", dict(missing=i)) for i in range(8)]
    out += [("negative rows", dict(n_rows=-1)), ("n_cols = 0", dict(n_cols=0)), ("n_chr = 0", dict(n_chr=0)),
            ("more chromosomes than windows", dict(n_chr=11)), ("max_p_normal = -0.1", dict(thr=-0.1)),
            ("max_p_normal = 1.5", dict(thr=1.5)), ("max_p_normal = nan", dict(thr=math.nan)),
            ("n_cols above the cap", dict(n_cols=FILTER_CAP + 1, n_chr=1)),
            ("order: the arguments before the cap", dict(n_cols=FILTER_CAP + 1, thr=2.0))]
    return out


def test_every_refusal_of_the_filter_entry_keeps_its_status_and_its_whole_message():
    cases = _filter_entry_cases()
    assert [cid for cid, _ in cases] == list(ENTRY["icv_copy_states_filter"])
    for cid, kw in cases:
        assert _filter_entry(**kw) == ENTRY["icv_copy_states_filter"][cid], cid

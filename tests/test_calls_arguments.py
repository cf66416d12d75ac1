"""The arguments of tl.cnv_segments, tl.cnv_states_filter, tl.cnv_pseudobulk and tl.cnv_score that are refused before any
GPU work: for every bad input the exception's type and its whole message, and per function an input with two faults that
shows which one is reported.  The four functions share their checks (the int8 call matrix, the group table, the integer
validator); the strings below are what each function raised when it still had its own copy of them.  The last part holds
the entry points of the library they call to their argument-error strings.  No test here needs a device."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

I8 = np.int8


def _adata(n=4, w=10, chr_pos=None, x=None, states=None, post=None, labels=None):
    from infercnvpy_amd._compat import SimpleAnnData

    labels = list("aabb")[:n] if labels is None else labels
    ad = SimpleAnnData(np.zeros((len(labels), 3), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.obsm["X_cnv_states"] = np.zeros((n, w), dtype=I8) if states is None else states
    ad.obsm["X_cnv_posterior_neutral"] = np.ones((n, w)) if post is None else post
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def _without(*keys):
    def make():
        ad = _adata()
        for k in keys:
            if k == "chr_pos":
                del ad.uns["cnv"]["chr_pos"]
            elif k == "cnv":
                del ad.uns["cnv"]
            else:
                del ad.obsm[k]
        return ad
    return make


CHR_POS = [
    ("chr_pos outside", {"chr1": 0, "chr2": 10}), ("chr_pos same window", {"chr1": 0, "chr2": 4, "chr3": 4}),
    ("chr_pos not at 0", {"chr1": 1, "chr2": 4}), ("chr_pos string", {"chr1": 0, "chr2": "x"}), ("chr_pos empty", {}),
    ("chr_pos list", [0, 4]),
]


def _cases(fn):
    """(id, () -> adata, keywords) of every bad input of the function ``fn``."""
    out = []
    if fn == "cnv_segments":
        out += [
            ("missing obsm key", _adata, {"use_rep": "other"}),
            ("missing cnv_key", _without("cnv"), {}),
            ("missing chr_pos", _without("chr_pos"), {}),
            ("1-D calls", lambda: _adata(states=np.zeros(4, dtype=I8)), {}),
            ("calls without a shape", lambda: _adata(states=[[0, 1]]), {}),
            ("float calls", lambda: _adata(states=np.zeros((4, 10))), {}),
            ("sparse calls", lambda: _adata(states=sp.csr_matrix((4, 10), dtype=np.float32)), {}),
            ("no rows", lambda: _adata(states=np.zeros((0, 10), dtype=I8)), {}),
            ("no windows", lambda: _adata(states=np.zeros((4, 0), dtype=I8)), {}),
        ]
        out += [(cid, (lambda c=c: _adata(chr_pos=c)), {}) for cid, c in CHR_POS]
        out += [(f"min_fraction={v!r}", _adata, {"min_fraction": v}) for v in (0, 1.5, -0.5, True, "x", None, float("nan"))]
        out += [(f"min_windows={v!r}", _adata, {"min_windows": v}) for v in (0, -3, 1.5, True, "x", None, float("inf"))]
        out += [("unknown groupby", _adata, {"groupby": "nope"}), ("no cnv_leiden", _adata, {"groupby": "cnv_leiden"})]
    elif fn == "cnv_states_filter":
        big = 1 << 22
        out += [
            ("missing obsm key", _adata, {"use_rep": "other"}),
            ("missing posterior", _adata, {"posterior_key": "other"}),
            ("missing cnv_key", _without("cnv"), {}),
            ("missing chr_pos", _without("chr_pos"), {}),
            ("1-D calls", lambda: _adata(states=np.zeros(4, dtype=I8)), {}),
            ("calls without a shape", lambda: _adata(states=[[0, 1]]), {}),
            ("float calls", lambda: _adata(states=np.zeros((4, 10))), {}),
            ("posterior of another shape", lambda: _adata(post=np.ones((4, 9))), {}),
            ("posterior without a shape", lambda: _adata(post=[[1.0]]), {}),
            ("float32 posterior", lambda: _adata(post=np.ones((4, 10), dtype=np.float32)), {}),
            ("no rows", lambda: _adata(states=np.zeros((0, 10), dtype=I8), post=np.ones((0, 10))), {}),
            ("no windows", lambda: _adata(states=np.zeros((4, 0), dtype=I8), post=np.ones((4, 0))), {}),
            ("W above the cap", lambda: _adata(states=np.zeros((1, big + 1), dtype=I8), post=np.zeros((1, big + 1)),
                                               chr_pos={"chr1": 0}), {}),
        ]
        out += [(cid, (lambda c=c: _adata(chr_pos=c)), {}) for cid, c in CHR_POS]
        out += [(f"max_p_normal={v!r}", _adata, {"max_p_normal": v}) for v in (-0.1, 1.5, True, "x", None, float("nan"))]
    elif fn == "cnv_pseudobulk":
        out += [
            ("missing obsm key", _adata, {"groupby": "clone", "use_rep": "other"}),
            ("missing cnv_key", _without("cnv"), {"groupby": "clone"}),
            ("missing chr_pos", _without("chr_pos"), {"groupby": "clone"}),
            ("unknown groupby", _adata, {"groupby": "nope"}),
            ("no cnv_leiden", _adata, {}),
            ("1-D X", lambda: _adata(x=np.ones(4)), {"groupby": "clone"}),
            ("X without a shape", lambda: _adata(x=[[1.0]]), {"groupby": "clone"}),
            ("no rows", lambda: _adata(x=np.ones((0, 10))), {"groupby": "clone"}),
            ("no windows", lambda: _adata(x=np.ones((4, 0))), {"groupby": "clone"}),
        ]
        out += [(f"min_cells={v!r}", _adata, {"groupby": "clone", "min_cells": v})
                for v in (0, -3, 1.5, True, "x", None, float("inf"))]
        out += [(cid, (lambda c=c: _adata(chr_pos=c)), {"groupby": "clone"}) for cid, c in CHR_POS]
        out += [
            ("labels of another length", lambda: _adata(labels=list("aabbc")), {"groupby": "clone"}),
            ("no group is large enough", _adata, {"groupby": "clone", "min_cells": 3}),
            ("every label is missing", lambda: _adata(labels=[None, np.nan, None, None]), {"groupby": "clone"}),
        ]
    else:
        out += [("no cnv_leiden", _adata, {}), ("no cnv_leiden, old keyword", _adata, {"obs_key": "cnv_leiden"})]
    return out


EXPECTED = {
    "cnv_segments": {
        'missing obsm key': (KeyError, 'tl.cnv_segments: X_other not found in adata.obsm. Did you run `tl.cnv_states`?'),
        'missing cnv_key': (KeyError, "tl.cnv_segments: chr_pos not found in adata.uns['cnv']. Did you run `tl.cnv_states`? (it reads what `tl.infercnv` leaves there)"),
        'missing chr_pos': (KeyError, "tl.cnv_segments: chr_pos not found in adata.uns['cnv']. Did you run `tl.cnv_states`? (it reads what `tl.infercnv` leaves there)"),
        '1-D calls': (ValueError, 'tl.cnv_segments: X_cnv_states must be 2-D'),
        'calls without a shape': (ValueError, 'tl.cnv_segments: X_cnv_states must be 2-D'),
        'float calls': (ValueError, 'tl.cnv_segments: X_cnv_states must be int8 (-1 loss, 0 neutral, +1 gain), not float64'),
        'sparse calls': (ValueError, 'tl.cnv_segments: X_cnv_states must be int8 (-1 loss, 0 neutral, +1 gain), not float32'),
        'no rows': (ValueError, 'tl.cnv_segments: empty matrix of shape (0, 10)'),
        'no windows': (ValueError, 'tl.cnv_segments: empty matrix of shape (4, 0)'),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'min_fraction=0': (ValueError, 'tl.cnv_segments: min_fraction=0 must lie in (0, 1]'),
        'min_fraction=1.5': (ValueError, 'tl.cnv_segments: min_fraction=1.5 must lie in (0, 1]'),
        'min_fraction=-0.5': (ValueError, 'tl.cnv_segments: min_fraction=-0.5 must lie in (0, 1]'),
        'min_fraction=True': (ValueError, 'tl.cnv_segments: min_fraction=True must lie in (0, 1]'),
        "min_fraction='x'": (ValueError, "tl.cnv_segments: min_fraction='x' must be a number in (0, 1]"),
        'min_fraction=None': (ValueError, 'tl.cnv_segments: min_fraction=None must be a number in (0, 1]'),
        'min_fraction=nan': (ValueError, 'tl.cnv_segments: min_fraction=nan must be a number in (0, 1]'),
        'min_windows=0': (ValueError, 'tl.cnv_segments: min_windows=0 must be an integer >= 1'),
        'min_windows=-3': (ValueError, 'tl.cnv_segments: min_windows=-3 must be an integer >= 1'),
        'min_windows=1.5': (ValueError, 'tl.cnv_segments: min_windows=1.5 must be an integer >= 1'),
        'min_windows=True': (ValueError, 'tl.cnv_segments: min_windows=True must be an integer >= 1'),
        "min_windows='x'": (ValueError, "tl.cnv_segments: min_windows='x' must be an integer >= 1"),
        'min_windows=None': (ValueError, 'tl.cnv_segments: min_windows=None must be an integer >= 1'),
        'min_windows=inf': (ValueError, 'tl.cnv_segments: min_windows=inf must be an integer >= 1'),
        'unknown groupby': (ValueError, 'tl.cnv_segments: `nope` not found in `adata.obs`'),
        'no cnv_leiden': (ValueError, 'tl.cnv_segments: `cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?'),
    },
    "cnv_states_filter": {
        'missing obsm key': (KeyError, 'tl.cnv_states_filter: X_other not found in adata.obsm. Did you run `tl.cnv_states`?'),
        'missing posterior': (KeyError, 'tl.cnv_states_filter: X_other_neutral not found in adata.obsm. Did you run `tl.cnv_posteriors`?'),
        'missing cnv_key': (KeyError, "tl.cnv_states_filter: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        'missing chr_pos': (KeyError, "tl.cnv_states_filter: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        '1-D calls': (ValueError, 'tl.cnv_states_filter: X_cnv_states must be 2-D'),
        'calls without a shape': (ValueError, 'tl.cnv_states_filter: X_cnv_states must be 2-D'),
        'float calls': (ValueError, 'tl.cnv_states_filter: X_cnv_states must be int8 (-1 loss, 0 neutral, +1 gain), not float64'),
        'posterior of another shape': (ValueError, 'tl.cnv_states_filter: X_cnv_posterior_neutral has shape (4, 9), X_cnv_states has (4, 10)'),
        'posterior without a shape': (ValueError, 'tl.cnv_states_filter: X_cnv_posterior_neutral has shape (), X_cnv_states has (4, 10)'),
        'float32 posterior': (ValueError, 'tl.cnv_states_filter: X_cnv_posterior_neutral must be float64, not float32'),
        'no rows': (ValueError, 'tl.cnv_states_filter: empty matrix of shape (0, 10)'),
        'no windows': (ValueError, 'tl.cnv_states_filter: empty matrix of shape (4, 0)'),
        'W above the cap': (ValueError, "tl.cnv_states_filter: 4194305 windows; a run's int64 sum takes at most 4194304"),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'max_p_normal=-0.1': (ValueError, 'tl.cnv_states_filter: max_p_normal=-0.1 must lie in [0, 1]'),
        'max_p_normal=1.5': (ValueError, 'tl.cnv_states_filter: max_p_normal=1.5 must lie in [0, 1]'),
        'max_p_normal=True': (ValueError, 'tl.cnv_states_filter: max_p_normal=True must lie in [0, 1]'),
        "max_p_normal='x'": (ValueError, "tl.cnv_states_filter: max_p_normal='x' must be a number in [0, 1]"),
        'max_p_normal=None': (ValueError, 'tl.cnv_states_filter: max_p_normal=None must be a number in [0, 1]'),
        'max_p_normal=nan': (ValueError, 'tl.cnv_states_filter: max_p_normal=nan must lie in [0, 1]'),
    },
    "cnv_pseudobulk": {
        'missing obsm key': (KeyError, 'tl.cnv_pseudobulk: X_other not found in adata.obsm. Did you run `tl.infercnv`?'),
        'missing cnv_key': (KeyError, "tl.cnv_pseudobulk: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        'missing chr_pos': (KeyError, "tl.cnv_pseudobulk: chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
        'unknown groupby': (KeyError, 'tl.cnv_pseudobulk: `nope` not found in `adata.obs`'),
        'no cnv_leiden': (KeyError, 'tl.cnv_pseudobulk: `cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?'),
        '1-D X': (ValueError, 'tl.cnv_pseudobulk: X_cnv must be 2-D'),
        'X without a shape': (ValueError, 'tl.cnv_pseudobulk: X_cnv must be 2-D'),
        'no rows': (ValueError, 'tl.cnv_pseudobulk: empty matrix of shape (0, 10)'),
        'no windows': (ValueError, 'tl.cnv_pseudobulk: empty matrix of shape (4, 0)'),
        'min_cells=0': (ValueError, 'tl.cnv_pseudobulk: min_cells=0 must be an integer >= 1'),
        'min_cells=-3': (ValueError, 'tl.cnv_pseudobulk: min_cells=-3 must be an integer >= 1'),
        'min_cells=1.5': (ValueError, 'tl.cnv_pseudobulk: min_cells=1.5 must be an integer >= 1'),
        'min_cells=True': (ValueError, 'tl.cnv_pseudobulk: min_cells=True must be an integer >= 1'),
        "min_cells='x'": (ValueError, "tl.cnv_pseudobulk: min_cells='x' must be an integer >= 1"),
        'min_cells=None': (ValueError, 'tl.cnv_pseudobulk: min_cells=None must be an integer >= 1'),
        'min_cells=inf': (ValueError, 'tl.cnv_pseudobulk: min_cells=inf must be an integer >= 1'),
        'chr_pos outside': (ValueError, 'tl.cnv_states: chr_pos start 10 is outside [0, 10)'),
        'chr_pos same window': (ValueError, 'tl.cnv_states: two chromosomes of chr_pos start at the same window'),
        'chr_pos not at 0': (ValueError, 'tl.cnv_states: no chromosome of chr_pos starts at window 0'),
        'chr_pos string': (ValueError, "tl.cnv_states: chr_pos start 'x' is not an integer"),
        'chr_pos empty': (ValueError, 'tl.cnv_states: chr_pos is empty'),
        'chr_pos list': (ValueError, 'tl.cnv_states: chr_pos must map chromosome names to their first window'),
        'labels of another length': (ValueError, 'tl.cnv_pseudobulk: `clone` has 5 labels for the 4 rows of X_cnv'),
        'no group is large enough': (ValueError, 'tl.cnv_pseudobulk: no group of `clone` has min_cells=3 cells'),
        'every label is missing': (ValueError, 'tl.cnv_pseudobulk: no group of `clone` has min_cells=1 cells'),
    },
    "cnv_score": {
        'no cnv_leiden': (ValueError, '`cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?'),
        'no cnv_leiden, old keyword': (ValueError, '`cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?'),
    },
}


@pytest.mark.parametrize("fn", list(EXPECTED))
def test_every_bad_input_keeps_its_exception_and_its_whole_message(fn):
    import infercnvpy_amd as cnv

    cases = _cases(fn)
    assert [cid for cid, _, _ in cases] == list(EXPECTED[fn])
    for cid, make, kw in cases:
        kind, message = EXPECTED[fn][cid]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", FutureWarning)  # (the renamed keyword of tl.cnv_score)
            with pytest.raises(kind) as info:
                getattr(cnv.tl, fn)(make(), **kw)
        assert type(info.value) is kind, (fn, cid)
        assert info.value.args[0] == message, (fn, cid)


# inputs that are wrong in two ways, along the order of each function's checks
ORDER = {
    "cnv_segments": [  # keys, chr_pos key, 2-D, int8, empty, chr_pos, min_fraction, min_windows, groupby
        (lambda: _without("chr_pos")(), {"use_rep": "other"}, KeyError, "X_other not found"),
        (lambda: _adata(chr_pos={}, states=np.zeros(4)), {}, ValueError, "must be 2-D"),
        (lambda: _adata(states=np.zeros((0, 10))), {}, ValueError, "must be int8"),
        (lambda: _adata(chr_pos={}, states=np.zeros((0, 10), dtype=I8)), {}, ValueError, "empty matrix"),
        (lambda: _adata(chr_pos={}), {"min_fraction": 0}, ValueError, "chr_pos is empty"),
        (_adata, {"min_fraction": 0, "min_windows": 0}, ValueError, "min_fraction=0"),
        (_adata, {"min_windows": 0, "groupby": "nope"}, ValueError, "min_windows=0"),
    ],
    "cnv_states_filter": [  # keys, 2-D, int8, posterior's shape and dtype, empty, cap, chr_pos, max_p_normal
        (_adata, {"use_rep": "other", "posterior_key": "other"}, KeyError, "X_other not found"),
        (lambda: _without("chr_pos")(), {"posterior_key": "other"}, KeyError, "X_other_neutral not found"),
        (lambda: _adata(states=np.zeros(4), post=np.ones(4)), {}, ValueError, "must be 2-D"),
        (lambda: _adata(states=np.zeros((4, 10)), post=np.ones((4, 9))), {}, ValueError, "must be int8"),
        (lambda: _adata(post=np.ones((4, 9), dtype=np.float32)), {}, ValueError, "has shape (4, 9)"),
        (lambda: _adata(states=np.zeros((0, 10), dtype=I8), post=np.ones((0, 10), dtype=np.float32)), {}, ValueError,
         "must be float64"),
        (lambda: _adata(states=np.zeros((0, 10), dtype=I8), post=np.ones((0, 10)), chr_pos={}), {}, ValueError,
         "empty matrix"),
        (lambda: _adata(chr_pos={}), {"max_p_normal": 2}, ValueError, "chr_pos is empty"),
    ],
    "cnv_pseudobulk": [  # keys, chr_pos key, groupby, 2-D, empty, min_cells, chr_pos, the group table
        (lambda: _without("chr_pos")(), {"use_rep": "other", "groupby": "nope"}, KeyError, "X_other not found"),
        (lambda: _without("chr_pos")(), {"groupby": "nope"}, KeyError, "chr_pos not found"),
        (lambda: _adata(x=np.ones(4)), {"groupby": "nope"}, KeyError, "`nope` not found"),
        (lambda: _adata(x=np.ones(4)), {"groupby": "clone", "min_cells": 0}, ValueError, "must be 2-D"),
        (lambda: _adata(x=np.ones((0, 10))), {"groupby": "clone", "min_cells": 0}, ValueError, "empty matrix"),
        (lambda: _adata(chr_pos={}), {"groupby": "clone", "min_cells": 0}, ValueError, "min_cells=0"),
        (lambda: _adata(chr_pos={}, labels=list("aabbc")), {"groupby": "clone"}, ValueError, "chr_pos is empty"),
        (lambda: _adata(labels=list("aabbc")), {"groupby": "clone", "min_cells": 9}, ValueError, "has 5 labels"),
    ],
    "cnv_score": [  # the renamed keyword is applied (and warned about) before the column is looked for
        (_adata, {"groupby": "clone", "obs_key": "cnv_leiden"}, ValueError, "`cnv_leiden` not found"),
    ],
}


@pytest.mark.parametrize("fn", list(ORDER))
def test_the_first_fault_in_the_order_of_the_checks_is_the_one_reported(fn):
    import infercnvpy_amd as cnv

    for make, kw, kind, part in ORDER[fn]:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", FutureWarning)
            with pytest.raises(kind) as info:
                getattr(cnv.tl, fn)(make(), **kw)
        assert type(info.value) is kind and part in info.value.args[0], (fn, part)


def test_cnv_score_warns_about_its_renamed_keyword_before_it_raises():
    import infercnvpy_amd as cnv

    with pytest.warns(FutureWarning, match="obs_key argument has been renamed to `groupby`"):
        with pytest.raises(ValueError):
            cnv.tl.cnv_score(_adata(), obs_key="cnv_leiden")


# ---- the library's entry points: status and icv_last_error() of every argument fault that is found before the device ----
ONE = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first


def _matrix(fmt="dense", dtype=0, n_rows=2, n_cols=5, ld=5, values=8, indptr=8):
    from infercnvpy_amd import _lib

    m = _lib.Matrix()
    m.format = {"dense": _lib.ICV_DENSE, "csr": _lib.ICV_CSR}.get(fmt, fmt)
    m.dtype, m.n_rows, m.n_cols, m.ld, m.values, m.indptr = dtype, n_rows, n_cols, ld, values, indptr
    return ctypes.byref(m)


def _hmm(name, *outputs, scalars=(2.0, 0.5, 0.999, 0.0005)):
    """(id, entry, arguments) of the faults that the three chain entry points report alike."""
    log = name == "icv_states_viterbi"
    good = (2.0, 0.5, -0.001, -7.0) if log else scalars
    none = (None,) * len(outputs)
    cap = 16384 if log else 4096
    rows = [
        ("no matrix", (None, ONE, 1, *good, *outputs)),
        ("no chr_start", (_matrix(), None, 1, *good, *outputs)),
        ("no outputs", (_matrix(), ONE, 1, *good, *none)),
        ("no chromosome", (_matrix(), ONE, 0, *good, *outputs)),
        ("negative rows", (_matrix(n_rows=-1), ONE, 1, *good, *outputs)),
        ("dtype 2", (_matrix(dtype=2), ONE, 1, *good, *outputs)),
        ("format 2", (_matrix(fmt=2), ONE, 1, *good, *outputs)),
        ("no windows", (_matrix(n_cols=0), ONE, 1, *good, *outputs)),
        ("windows above the cap", (_matrix(n_cols=cap + 1, ld=cap + 1), ONE, 1, *good, *outputs)),
        ("more chromosomes than windows", (_matrix(), ONE, 6, *good, *outputs)),
        ("amplitude 0", (_matrix(), ONE, 1, 0.0, *good[1:], *outputs)),
        ("h infinite", (_matrix(), ONE, 1, good[0], float("inf"), *good[2:], *outputs)),
        ("dense ld below n_cols", (_matrix(ld=4), ONE, 1, *good, *outputs)),
        ("dense without values", (_matrix(values=None), ONE, 1, *good, *outputs)),
        ("csr without indptr", (_matrix(fmt="csr", indptr=None), ONE, 1, *good, *outputs)),
        ("too many rows", (_matrix(n_rows=1 << 31), ONE, 1, *good, *outputs)),
        # the order: the shape before the parameters, the parameters before the matrix's pointers
        ("no windows and amplitude 0", (_matrix(n_cols=0), ONE, 1, 0.0, *good[1:], *outputs)),
        ("amplitude 0 and no values", (_matrix(values=None), ONE, 1, 0.0, *good[1:], *outputs)),
        ("no values and too many rows", (_matrix(values=None, n_rows=1 << 31), ONE, 1, *good, *outputs)),
    ]
    if not log:
        rows += [("pw 0.5", (_matrix(), ONE, 1, 2.0, 0.5, 0.5, 0.5, *outputs)),
                 ("pw denormal", (_matrix(), ONE, 1, 2.0, 0.5, 0.999, 5e-324, *outputs))]
    else:
        rows += [("stay infinite", (_matrix(), ONE, 1, 2.0, 0.5, float("-inf"), -7.0, *outputs))]
    return [(f"{name[4:]}: {cid}", name, (*args, None)) for cid, args in rows]


def _abi_cases():
    out = [
        ("states_rowsq: no matrix", "icv_states_rowsq", (None, ONE, ONE, None)),
        ("states_rowsq: no rowsq", "icv_states_rowsq", (_matrix(), None, ONE, None)),
        ("states_rowsq: no flag", "icv_states_rowsq", (_matrix(), ONE, None, None)),
        ("states_rowsq: negative rows", "icv_states_rowsq", (_matrix(n_rows=-1), ONE, ONE, None)),
        ("states_rowsq: negative windows", "icv_states_rowsq", (_matrix(n_cols=-1), ONE, ONE, None)),
        ("states_rowsq: dtype 2", "icv_states_rowsq", (_matrix(dtype=2), ONE, ONE, None)),
        ("states_rowsq: format 2", "icv_states_rowsq", (_matrix(fmt=2), ONE, ONE, None)),
        ("states_rowsq: dense ld below n_cols", "icv_states_rowsq", (_matrix(ld=4), ONE, ONE, None)),
    ]
    out += _hmm("icv_states_viterbi", ONE, ONE)
    out += _hmm("icv_posterior_chains", ONE, ONE, ONE)
    out += [("posterior_chains: loss without gain", "icv_posterior_chains",
             (_matrix(), ONE, 1, 2.0, 0.5, 0.999, 0.0005, ONE, ONE, None, None))]
    out += _hmm("icv_posterior_stats", ONE)
    gp = "icv_group_profiles"
    out += [
        ("group_profiles: no matrix", gp, (None, ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: negative list", gp, (_matrix(), ONE, -1, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: no rows listed", gp, (_matrix(), None, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: no group_ptr", gp, (_matrix(), ONE, 2, None, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: negative groups", gp, (_matrix(), ONE, 2, ONE, -1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: no sum", gp, (_matrix(), ONE, 2, ONE, 1, 40, None, ONE, ONE, None)),
        ("group_profiles: no stored", gp, (_matrix(), ONE, 2, ONE, 1, 40, ONE, None, ONE, None)),
        ("group_profiles: no flags", gp, (_matrix(), ONE, 2, ONE, 1, 40, ONE, ONE, None, None)),
        ("group_profiles: negative shift", gp, (_matrix(), ONE, 2, ONE, 1, -1, ONE, ONE, ONE, None)),
        ("group_profiles: shift 41", gp, (_matrix(), ONE, 2, ONE, 1, 41, ONE, ONE, ONE, None)),
        ("group_profiles: negative rows", gp, (_matrix(n_rows=-1), ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: no windows", gp, (_matrix(n_cols=0), ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: dtype 2", gp, (_matrix(dtype=2), ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: format 2", gp, (_matrix(fmt=2), ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
        ("group_profiles: dense ld below n_cols", gp, (_matrix(ld=4), ONE, 2, ONE, 1, 40, ONE, ONE, ONE, None)),
    ]
    gr = "icv_gram_f64"
    out += [
        ("gram_f64: no matrix", gr, (None, 1, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: no g", gr, (_matrix(), 1, ONE, 64, None, 5, 0, None)),
        ("gram_f64: negative rows", gr, (_matrix(n_rows=-1), 1, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: no columns", gr, (_matrix(n_cols=0), 1, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: ldg below n_cols", gr, (_matrix(), 1, ONE, 64, ONE, 4, 0, None)),
        ("gram_f64: panel dtype 2", gr, (_matrix(), 2, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: dtype 2", gr, (_matrix(dtype=2), 1, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: format 2", gr, (_matrix(fmt=2), 1, ONE, 64, ONE, 5, 0, None)),
        ("gram_f64: no panel", gr, (_matrix(), 1, None, 64, ONE, 5, 0, None)),
        ("gram_f64: panel stride 63", gr, (_matrix(), 1, ONE, 63, ONE, 5, 0, None)),
        ("gram_f64: panel stride 64 for 65 columns", gr, (_matrix(n_cols=65, ld=65), 1, ONE, 64, ONE, 65, 0, None)),
        ("gram_f64: format 2 and no panel", gr, (_matrix(fmt=2), 1, None, 64, ONE, 5, 0, None)),
    ]
    pr = "icv_project"
    out += [
        ("project: no matrix", pr, (None, ONE, 3, None, 0, ONE, 3, None)),
        ("project: no v", pr, (_matrix(), None, 3, None, 0, ONE, 3, None)),
        ("project: no out", pr, (_matrix(), ONE, 3, None, 0, None, 3, None)),
        ("project: no components", pr, (_matrix(), ONE, 0, None, 0, ONE, 3, None)),
        ("project: ldo below k", pr, (_matrix(), ONE, 3, None, 0, ONE, 2, None)),
        ("project: negative rows", pr, (_matrix(n_rows=-1), ONE, 3, None, 0, ONE, 3, None)),
        ("project: out dtype 2", pr, (_matrix(), ONE, 3, None, 2, ONE, 3, None)),
        ("project: dtype 2", pr, (_matrix(dtype=2), ONE, 3, None, 0, ONE, 3, None)),
        ("project: format 2", pr, (_matrix(fmt=2), ONE, 3, None, 0, ONE, 3, None)),
        ("project: no rows", pr, (_matrix(n_rows=0), ONE, 3, None, 0, ONE, 3, None)),
    ]
    sc, sf = "icv_segments_count", "icv_segments_fill"
    out += [
        ("segments_count: no states", sc, (None, 1, 5, ONE, 1, ONE, ONE, None)),
        ("segments_count: no chr_start", sc, (ONE, 1, 5, None, 1, ONE, ONE, None)),
        ("segments_count: negative rows", sc, (ONE, -1, 5, ONE, 1, ONE, ONE, None)),
        ("segments_count: no windows", sc, (ONE, 1, 0, ONE, 1, ONE, ONE, None)),
        ("segments_count: no chromosome", sc, (ONE, 1, 5, ONE, 0, ONE, ONE, None)),
        ("segments_count: more chromosomes than windows", sc, (ONE, 1, 5, ONE, 6, ONE, ONE, None)),
        ("segments_count: no counts", sc, (ONE, 1, 5, ONE, 1, None, ONE, None)),
        ("segments_count: no flag", sc, (ONE, 1, 5, ONE, 1, ONE, None, None)),
        ("segments_fill: no states", sf, (None, 1, 5, ONE, 1, ONE, 3, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: no chr_start", sf, (ONE, 1, 5, None, 1, ONE, 3, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: more chromosomes than windows", sf, (ONE, 1, 5, ONE, 6, ONE, 3, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: no offsets", sf, (ONE, 1, 5, ONE, 1, None, 3, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: negative segments", sf, (ONE, 1, 5, ONE, 1, ONE, -1, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: no seg_row", sf, (ONE, 1, 5, ONE, 1, ONE, 3, None, ONE, ONE, ONE, None)),
        ("segments_fill: no seg_state", sf, (ONE, 1, 5, ONE, 1, ONE, 3, ONE, ONE, ONE, None, None)),
        ("segments_fill: no segments", sf, (ONE, 1, 5, ONE, 1, ONE, 0, None, None, None, None, None)),
        ("segments_fill: no rows", sf, (ONE, 0, 5, ONE, 1, ONE, 3, ONE, ONE, ONE, ONE, None)),
        ("segments_fill: too many rows", sf, (ONE, 1 << 33, 5, ONE, 1, ONE, 3, ONE, ONE, ONE, ONE, None)),
    ]
    return out


ABI_EXPECTED = {
    'states_rowsq: no matrix': (1, 'bad states_rowsq arguments'),
    'states_rowsq: no rowsq': (1, 'bad states_rowsq arguments'),
    'states_rowsq: no flag': (1, 'bad states_rowsq arguments'),
    'states_rowsq: negative rows': (1, 'bad states_rowsq arguments'),
    'states_rowsq: negative windows': (1, 'bad states_rowsq arguments'),
    'states_rowsq: dtype 2': (1, 'bad states_rowsq arguments'),
    'states_rowsq: format 2': (1, 'bad states_rowsq arguments'),
    'states_rowsq: dense ld below n_cols': (1, 'bad states_rowsq arguments'),
    'states_viterbi: no matrix': (1, 'bad states_viterbi arguments'),
    'states_viterbi: no chr_start': (1, 'bad states_viterbi arguments'),
    'states_viterbi: no outputs': (1, 'bad states_viterbi arguments'),
    'states_viterbi: no chromosome': (1, 'bad states_viterbi arguments'),
    'states_viterbi: negative rows': (1, 'bad states_viterbi arguments'),
    'states_viterbi: dtype 2': (1, 'bad states_viterbi arguments'),
    'states_viterbi: format 2': (1, 'bad states_viterbi arguments'),
    'states_viterbi: no windows': (1, 'states_viterbi: n_cols = 0 must lie in [1, 16384] (9 bytes of LDS per window)'),
    'states_viterbi: windows above the cap': (1, 'states_viterbi: n_cols = 16385 must lie in [1, 16384] (9 bytes of LDS per window)'),
    'states_viterbi: more chromosomes than windows': (1, 'states_viterbi: more chromosomes than windows'),
    'states_viterbi: amplitude 0': (1, 'states_viterbi: amplitude and h must be finite and > 0, stay and sw finite'),
    'states_viterbi: h infinite': (1, 'states_viterbi: amplitude and h must be finite and > 0, stay and sw finite'),
    'states_viterbi: dense ld below n_cols': (1, 'states_viterbi: incomplete matrix'),
    'states_viterbi: dense without values': (1, 'states_viterbi: incomplete matrix'),
    'states_viterbi: csr without indptr': (1, 'states_viterbi: incomplete matrix'),
    'states_viterbi: too many rows': (2, 'states_viterbi: more than 2^31 - 1 rows in one call'),
    'states_viterbi: no windows and amplitude 0': (1, 'states_viterbi: n_cols = 0 must lie in [1, 16384] (9 bytes of LDS per window)'),
    'states_viterbi: amplitude 0 and no values': (1, 'states_viterbi: amplitude and h must be finite and > 0, stay and sw finite'),
    'states_viterbi: no values and too many rows': (1, 'states_viterbi: incomplete matrix'),
    'states_viterbi: stay infinite': (1, 'states_viterbi: amplitude and h must be finite and > 0, stay and sw finite'),
    'posterior_chains: no matrix': (1, 'bad posterior_chains arguments'),
    'posterior_chains: no chr_start': (1, 'bad posterior_chains arguments'),
    'posterior_chains: no outputs': (1, 'bad posterior_chains arguments'),
    'posterior_chains: no chromosome': (1, 'bad posterior_chains arguments'),
    'posterior_chains: negative rows': (1, 'bad posterior_chains arguments'),
    'posterior_chains: dtype 2': (1, 'bad posterior_chains arguments'),
    'posterior_chains: format 2': (1, 'bad posterior_chains arguments'),
    'posterior_chains: no windows': (1, 'posterior_chains: n_cols = 0 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_chains: windows above the cap': (1, 'posterior_chains: n_cols = 4097 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_chains: more chromosomes than windows': (1, 'posterior_chains: more chromosomes than windows'),
    'posterior_chains: amplitude 0': (1, 'posterior_chains: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_chains: h infinite': (1, 'posterior_chains: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_chains: dense ld below n_cols': (1, 'posterior_chains: incomplete matrix'),
    'posterior_chains: dense without values': (1, 'posterior_chains: incomplete matrix'),
    'posterior_chains: csr without indptr': (1, 'posterior_chains: incomplete matrix'),
    'posterior_chains: too many rows': (2, 'posterior_chains: more than 2^31 - 1 rows in one call'),
    'posterior_chains: no windows and amplitude 0': (1, 'posterior_chains: n_cols = 0 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_chains: amplitude 0 and no values': (1, 'posterior_chains: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_chains: no values and too many rows': (1, 'posterior_chains: incomplete matrix'),
    'posterior_chains: pw 0.5': (1, 'posterior_chains: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_chains: pw denormal': (1, 'posterior_chains: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_chains: loss without gain': (1, 'bad posterior_chains arguments'),
    'posterior_stats: no matrix': (1, 'bad posterior_stats arguments'),
    'posterior_stats: no chr_start': (1, 'bad posterior_stats arguments'),
    'posterior_stats: no outputs': (1, 'bad posterior_stats arguments'),
    'posterior_stats: no chromosome': (1, 'bad posterior_stats arguments'),
    'posterior_stats: negative rows': (1, 'bad posterior_stats arguments'),
    'posterior_stats: dtype 2': (1, 'bad posterior_stats arguments'),
    'posterior_stats: format 2': (1, 'bad posterior_stats arguments'),
    'posterior_stats: no windows': (1, 'posterior_stats: n_cols = 0 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_stats: windows above the cap': (1, 'posterior_stats: n_cols = 4097 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_stats: more chromosomes than windows': (1, 'posterior_stats: more chromosomes than windows'),
    'posterior_stats: amplitude 0': (1, 'posterior_stats: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_stats: h infinite': (1, 'posterior_stats: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_stats: dense ld below n_cols': (1, 'posterior_stats: incomplete matrix'),
    'posterior_stats: dense without values': (1, 'posterior_stats: incomplete matrix'),
    'posterior_stats: csr without indptr': (1, 'posterior_stats: incomplete matrix'),
    'posterior_stats: too many rows': (2, 'posterior_stats: more than 2^31 - 1 rows in one call'),
    'posterior_stats: no windows and amplitude 0': (1, 'posterior_stats: n_cols = 0 must lie in [1, 4096] (32 bytes of LDS per window)'),
    'posterior_stats: amplitude 0 and no values': (1, 'posterior_stats: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_stats: no values and too many rows': (1, 'posterior_stats: incomplete matrix'),
    'posterior_stats: pw 0.5': (1, 'posterior_stats: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'posterior_stats: pw denormal': (1, 'posterior_stats: amplitude and h must be finite and > 0, ps = 1 - p and pw = p / 2 for a p in (0, 1) with pw a normal float64'),
    'group_profiles: no matrix': (1, 'bad group_profiles arguments'),
    'group_profiles: negative list': (1, 'bad group_profiles arguments'),
    'group_profiles: no rows listed': (1, 'bad group_profiles arguments'),
    'group_profiles: no group_ptr': (1, 'bad group_profiles arguments'),
    'group_profiles: negative groups': (1, 'bad group_profiles arguments'),
    'group_profiles: no sum': (1, 'bad group_profiles arguments'),
    'group_profiles: no stored': (1, 'bad group_profiles arguments'),
    'group_profiles: no flags': (1, 'bad group_profiles arguments'),
    'group_profiles: negative shift': (1, 'bad group_profiles arguments'),
    'group_profiles: shift 41': (1, 'bad group_profiles arguments'),
    'group_profiles: negative rows': (1, 'bad group_profiles arguments'),
    'group_profiles: no windows': (1, 'bad group_profiles arguments'),
    'group_profiles: dtype 2': (1, 'bad group_profiles arguments'),
    'group_profiles: format 2': (1, 'bad group_profiles arguments'),
    'group_profiles: dense ld below n_cols': (1, 'bad group_profiles arguments'),
    'gram_f64: no matrix': (1, 'bad gram_f64 arguments'),
    'gram_f64: no g': (1, 'bad gram_f64 arguments'),
    'gram_f64: negative rows': (1, 'bad gram_f64 arguments'),
    'gram_f64: no columns': (1, 'bad gram_f64 arguments'),
    'gram_f64: ldg below n_cols': (1, 'bad gram_f64 arguments'),
    'gram_f64: panel dtype 2': (1, 'bad gram_f64 arguments'),
    'gram_f64: dtype 2': (1, 'bad gram_f64 arguments'),
    'gram_f64: format 2': (1, 'bad gram_f64 arguments'),
    'gram_f64: no panel': (1, 'gram_f64: the panel needs a row stride of at least n_cols rounded up to 64'),
    'gram_f64: panel stride 63': (1, 'gram_f64: the panel needs a row stride of at least n_cols rounded up to 64'),
    'gram_f64: panel stride 64 for 65 columns': (1, 'gram_f64: the panel needs a row stride of at least n_cols rounded up to 64'),
    'gram_f64: format 2 and no panel': (1, 'bad gram_f64 arguments'),
    'project: no matrix': (1, 'bad project arguments'),
    'project: no v': (1, 'bad project arguments'),
    'project: no out': (1, 'bad project arguments'),
    'project: no components': (1, 'bad project arguments'),
    'project: ldo below k': (1, 'bad project arguments'),
    'project: negative rows': (1, 'bad project arguments'),
    'project: out dtype 2': (1, 'bad project arguments'),
    'project: dtype 2': (1, 'bad project arguments'),
    'project: format 2': (1, 'bad project arguments'),
    'project: no rows': (0, ''),
    'segments_count: no states': (1, 'bad segments_count arguments'),
    'segments_count: no chr_start': (1, 'bad segments_count arguments'),
    'segments_count: negative rows': (1, 'bad segments_count arguments'),
    'segments_count: no windows': (1, 'bad segments_count arguments'),
    'segments_count: no chromosome': (1, 'bad segments_count arguments'),
    'segments_count: more chromosomes than windows': (1, 'bad segments_count arguments'),
    'segments_count: no counts': (1, 'bad segments_count arguments'),
    'segments_count: no flag': (1, 'bad segments_count arguments'),
    'segments_fill: no states': (1, 'bad segments_fill arguments'),
    'segments_fill: no chr_start': (1, 'bad segments_fill arguments'),
    'segments_fill: more chromosomes than windows': (1, 'bad segments_fill arguments'),
    'segments_fill: no offsets': (1, 'bad segments_fill arguments'),
    'segments_fill: negative segments': (1, 'bad segments_fill arguments'),
    'segments_fill: no seg_row': (1, 'bad segments_fill arguments'),
    'segments_fill: no seg_state': (1, 'bad segments_fill arguments'),
    'segments_fill: no segments': (0, ''),
    'segments_fill: no rows': (0, ''),
    'segments_fill: too many rows': (2, 'segments_fill: too many rows for one call'),
}


def test_every_argument_fault_of_the_entry_points_keeps_its_status_and_its_whole_message():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    cases = _abi_cases()
    assert [cid for cid, _, _ in cases] == list(ABI_EXPECTED)
    for cid, entry, args in cases:
        status, message = ABI_EXPECTED[cid]
        assert getattr(lib, entry)(*args) == status, cid
        if status != _lib.ICV_OK:
            assert lib.icv_last_error().decode() == message, cid

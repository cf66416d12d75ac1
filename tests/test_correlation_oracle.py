"""The oracle of tl.cnv_correlation and tl.cnv_signal (tests/_correlation_oracle.py) against numpy's
corrcoef, its degenerate cases, the planted tumour / normal case, the top-row rule, and everything the two functions and
their two entry points refuse before they touch the device.  No GPU."""
import ctypes
import fractions
import functools
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _correlation_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle against numpy --------------------------------------------------------------------------------------------------
def _rows(n, w, density, seed):
    """n rows of normal values at the density, at least two stored values in every row."""
    rng = np.random.default_rng(seed)
    keep = rng.random((n, w)) < density
    keep[:, :2] = True
    return rng.normal(0.0, 0.5, (n, w)) * keep


@pytest.mark.parametrize("w", [63, 64, 65, 270, 1802])
@pytest.mark.parametrize("density", [0.05, 0.13, 1.0])
def test_the_oracle_agrees_with_corrcoef(w, density):
    """The three chains of length W have a forward error of about 4 W 2^-53 (8e-13 at W = 1802) for rows with
    |mean| <= std; the bound of the test is 1e-12 absolute."""
    x = _rows(5, w, density, 100 + w)
    p = np.random.default_rng(w).normal(0.0, 0.3, (3, w))
    assert (np.abs(x.mean(axis=1)) <= x.std(axis=1)).all()
    got = co.correlate(x, p)
    want = np.corrcoef(np.vstack([x, p]))[:5, 5:]
    err = float(np.abs(got["r"] - want).max())
    print(f"W={w} density={density}: max |r - corrcoef| = {err:.3g}")
    assert err <= 1e-12
    assert np.abs(got["signal"] - (x * x).mean(axis=1)).max() <= 1e-12
    assert np.array_equal(got["best_g"], np.argmax(got["r"], axis=1))
    assert np.array_equal(got["best_r"], got["r"][np.arange(5), got["best_g"]])


def test_host_steps_are_fsum_and_one_rounding_each():
    p = np.asarray([[1e16, 1.0, -1e16, 3.0], [0.1, 0.2, 0.3, 0.4]])
    c, s2 = co.centre(p)
    assert c[0].tolist() == [1e16 - 1.0, 0.0, -1e16 - 1.0, 2.0]  # (the mean is fsum / W = 1.0: a naive sum gives 0.75)
    m = float(fractions.Fraction(0.1) + fractions.Fraction(0.2) + fractions.Fraction(0.3) + fractions.Fraction(0.4)) / 4
    assert c[1].tolist() == [v - m for v in p[1]]
    assert s2[1] == float(sum(fractions.Fraction(float(v * v)) for v in c[1]))
    # the package's host steps are the oracle's
    from infercnvpy_amd.tl._correlation import centre_profiles

    q = np.random.default_rng(0).normal(0.0, 0.3, (4, 1802))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(centre_profiles(q), co.centre(q)))


# ---- degenerate cases ----------------------------------------------------------------------------------------------------------
def test_degenerate_rows_and_profiles_are_nan():
    x = np.asarray([[0.0, 0.0, 0.0, 0.0], [0.5, 0.5, 0.5, 0.5], [0.1, -0.2, 0.3, 0.0]])
    p = np.asarray([[1.0, 2.0, 3.0, 4.0], [7.0, 7.0, 7.0, 7.0]])
    got = co.correlate(x, p)
    assert np.isnan(got["r"][0]).all() and np.isnan(got["r"][1]).all()  # an empty row, a constant row
    assert np.isnan(got["r"][:, 1]).all() and not np.isnan(got["r"][2, 0])  # a constant profile
    assert got["best_g"].tolist() == [-1, -1, 0] and np.isnan(got["best_r"][:2]).all()
    assert got["signal"].tolist() == [0.0, 0.25, (0.1 * 0.1 + 0.2 * 0.2 + 0.3 * 0.3) / 4]
    one = co.correlate(np.asarray([[0.7], [0.0]]), np.asarray([[1.5]]))  # W = 1
    assert np.isnan(one["r"]).all() and one["best_g"].tolist() == [-1, -1] and one["signal"].tolist() == [0.7 * 0.7, 0.0]
    none = co.correlate(x, np.zeros((0, 4)))  # G = 0
    assert none["r"].shape == (3, 0) and none["best_g"].tolist() == [-1, -1, -1] and np.isnan(none["best_r"]).all()
    assert none["signal"].tobytes() == got["signal"].tobytes()


def test_ties_go_to_the_lower_profile_and_r_is_clipped():
    x = np.asarray([[1.0, 2.0, 4.5], [3.0, -1.0, 0.5]])
    p = np.asarray([[3.0, 1.0, 0.0], [1.0, 2.0, 4.0], [1.0, 2.0, 4.0]])
    got = co.correlate(x, p)
    assert got["r"][0, 1] == got["r"][0, 2] > got["r"][0, 0] and got["best_g"][0] == 1
    r = np.asarray([[np.nan, 0.25, 0.25], [-0.0, 0.0, np.nan], [np.nan, np.nan, -1.0]])
    best_r, best_g = co.best(r)
    assert best_g.tolist() == [1, 0, 2] and best_r.tolist() == [0.25, -0.0, -1.0] and np.signbit(best_r[1])
    # D / sqrt(vx s2) = 2, -2 and 0.5 with vx = 1 and s2 = 1
    _, r = co.finish(np.zeros(3), np.ones(3), np.asarray([[2.0], [-2.0], [0.5]]), np.ones(1), 4)
    assert r.ravel().tolist() == [1.0, -1.0, 0.5]


# ---- order independence --------------------------------------------------------------------------------------------------------
def test_storage_and_stored_zeros_change_no_byte():
    rng = np.random.default_rng(4)
    dense = rng.normal(0.0, 0.5, (9, 70)) * (rng.random((9, 70)) < 0.3)
    p = rng.normal(0.0, 0.3, (4, 70))
    want = co.correlate(dense, p)
    csr = sp.csr_matrix(dense)
    filler = np.where(np.arange(dense.size) % 2 == 0, 0.0, -0.0).reshape(dense.shape)  # every entry stored: 0.0 and -0.0
    zeros = sp.csr_matrix((np.where(dense == 0, filler, dense).ravel(), np.tile(np.arange(70), 9), np.arange(10) * 70),
                          shape=(9, 70))
    assert zeros.nnz == 9 * 70 and np.signbit(zeros.data[zeros.data == 0]).any() and (zeros.toarray() == dense).all()
    forms = {"csr": csr, "csc": csr.tocsc(), "fortran": np.asfortranarray(dense), "stored_zeros": zeros,
             "float32": csr.astype(np.float32)}
    for name, x in forms.items():
        ref = want if name != "float32" else co.correlate(dense.astype(np.float32).astype(np.float64), p)
        got = co.correlate(x, p)
        for k in ("A", "B", "signal", "r", "best_r"):
            assert co.same_bytes(got[k], ref[k]), (name, k)
        assert np.array_equal(got["best_g"], ref["best_g"]), name


# ---- the planted case ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_scores(seed):
    c = co.planted(seed)
    rows, profile = co.top_profile(c["x"], 0.05)
    top = co.correlate(c["x"], profile)
    means = np.stack([c["x"][c["clone"] == g].mean(axis=0) for g in range(3)])
    return c, rows, top, co.correlate(c["x"], means)


def test_the_correlation_separates_tumour_from_normal_where_the_signal_does_not():
    """3 x 48 tumour cells (a shared trunk, one private event per clone) and 96 normal cells, 270 windows, noise 0.3,
    shifts of +-0.3, seeds 0-4: r against the top-5 % profile separates the two (tumour cells outside the top rows
    >= 0.269, normal cells <= 0.150), the signal alone separates them in none of the five seeds."""
    overlap = 0
    for seed in range(5):
        c, rows, top, _ = planted_scores(seed)
        tumour = c["clone"] >= 0
        outside = np.ones(240, dtype=bool)
        outside[rows] = False
        assert rows.shape == (13,) and tumour[rows].all()  # (0.05 as a float64 is above 1/20: ceil gives 13)
        r = top["r"][:, 0]
        print(f"seed {seed}: tumour r >= {r[tumour & outside].min():.3f}, normal r <= {r[~tumour].max():.3f}; "
              f"tumour signal >= {top['signal'][tumour].min():.4f}, normal signal <= {top['signal'][~tumour].max():.4f}")
        assert r[tumour & outside].min() > r[~tumour].max()
        overlap += bool(top["signal"][~tumour].max() > top["signal"][tumour].min())
    assert overlap >= 1


def test_the_arg_max_over_the_clone_means_is_the_planted_clone():
    for seed in range(5):
        c, _, _, clones = planted_scores(seed)
        tumour = c["clone"] >= 0
        assert np.array_equal(clones["best_g"][tumour], c["clone"][tumour]), seed


# ---- the top rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top_fraction, n, k", [(0.05, 240, 13), ("1/20", 240, 12), (fractions.Fraction(1, 20), 241, 13),
                                                (0.5, 3, 2), (1, 7, 7), (1.0, 7, 7), (1e-9, 10, 1), (0.25, 8, 2)])
def test_the_number_of_top_rows(top_fraction, n, k):
    from infercnvpy_amd.tl import _correlation

    assert co.top_count(top_fraction, n) == k
    assert _correlation.top_count("who", top_fraction, n) == (k, fractions.Fraction(top_fraction))


def test_ties_of_the_signal_go_to_the_lower_row():
    assert co.top_rows([1.0, 3.0, 3.0, 2.0, 3.0], "2/5").tolist() == [1, 2]
    assert co.top_rows([1.0, 3.0, 3.0, 2.0, 3.0], "4/5").tolist() == [1, 2, 3, 4]
    assert co.top_rows([0.0, 0.0, 0.0], 0.1).tolist() == [0]
    # the device's selection: a stable descending sort
    torch = pytest.importorskip("torch")
    signal = torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0], dtype=torch.float64)
    assert sorted(torch.sort(signal, descending=True, stable=True)[1][:2].tolist()) == [1, 2]


# ---- the library and the package, as far as they go without a GPU -----------------------------------------------------------
def test_symbols_are_exported_and_declared():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    for name in ("icv_profile_corr", "icv_profile_corr_best"):
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("cnv_correlation", "cnv_signal"):
        assert name in cnv.tl.__all__ and callable(getattr(cnv.tl, name))


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld, m.values = _lib.ICV_DENSE, _lib.ICV_F64, 4, 5, 5, 8
    ref = ctypes.byref(m)
    corr = lib.icv_profile_corr
    assert corr(None, one, one, 1, one, one, one, one, one, None) == bad
    assert corr(ref, None, one, 1, one, one, one, one, one, None) == bad
    assert corr(ref, one, None, 1, one, one, one, one, one, None) == bad
    assert corr(ref, one, one, -1, one, one, one, one, one, None) == bad
    assert corr(ref, one, one, 1, None, one, one, one, one, None) == bad
    assert corr(ref, one, one, 1, one, None, one, one, one, None) == bad
    assert corr(ref, one, one, 1, one, one, None, one, one, None) == bad
    assert corr(ref, one, one, 1, one, one, one, None, one, None) == bad
    assert corr(ref, one, one, 1, one, one, one, one, None, None) == bad
    assert corr(ref, None, None, 0, None, one, one, None, one, None) == bad  # (G = 0 still needs a, b and signal)
    for field, value in (("n_cols", 0), ("n_rows", -1), ("dtype", 7), ("format", 7), ("ld", 4), ("values", None)):
        keep = getattr(m, field)
        setattr(m, field, value)
        assert corr(ref, one, one, 1, one, one, one, one, one, None) == bad, field
        setattr(m, field, keep)
    m.format, m.indptr = _lib.ICV_CSR, None
    assert corr(ref, one, one, 1, one, one, one, one, one, None) == bad  # a CSR matrix without row offsets
    assert b"profile_corr" in lib.icv_last_error()
    best = lib.icv_profile_corr_best
    assert best(None, 1, 1, one, one, None) == bad
    assert best(one, 1, 1, None, one, None) == bad
    assert best(one, 1, 1, one, None, None) == bad
    assert best(one, -1, 1, one, one, None) == bad
    assert best(one, 1, -1, one, one, None) == bad
    assert best(one, 1, 2 ** 31, one, one, None) == bad
    assert best(None, 0, 3, None, None, None) == _lib.ICV_OK  # no rows: nothing runs


# ---- what the two functions refuse before they touch the device -----------------------------------------------------------------
def _adata(n=6, w=10, x=None, labels=None):
    from infercnvpy_amd._compat import SimpleAnnData

    labels = list("aabbcc")[:n] if labels is None else labels
    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4}}
    return ad


def _container(w=10, key="X_cnv"):
    from infercnvpy_amd._compat import SimpleAnnData

    p = np.arange(2.0 * w).reshape(2, w)
    return SimpleAnnData(p, obs=pd.DataFrame(index=["a", "b"]), obsm={key: p})


NAN_PROFILE = np.asarray([[0.0] * 9 + [np.nan]])
BAD = [
    ("missing obsm key", {"use_rep": "other"}, KeyError,
     "tl.cnv_correlation: X_other not found in adata.obsm. Did you run `tl.infercnv`?"),
    ("profiles and groupby", {"profiles": np.zeros((1, 10)), "groupby": "clone"}, ValueError,
     "tl.cnv_correlation: give `profiles` or `groupby`, not both"),
    ("top_fraction=0", {"top_fraction": 0}, ValueError, "tl.cnv_correlation: top_fraction=0 must lie in (0, 1]"),
    ("top_fraction=1.5", {"top_fraction": 1.5}, ValueError, "tl.cnv_correlation: top_fraction=1.5 must lie in (0, 1]"),
    ("top_fraction=nan", {"top_fraction": float("nan")}, ValueError,
     "tl.cnv_correlation: top_fraction=nan must be a number in (0, 1]"),
    ("top_fraction=True", {"top_fraction": True}, ValueError, "tl.cnv_correlation: top_fraction=True must lie in (0, 1]"),
    ("top_fraction='x'", {"top_fraction": "x"}, ValueError,
     "tl.cnv_correlation: top_fraction='x' must be a number in (0, 1]"),
    ("width mismatch", {"profiles": np.zeros((2, 9))}, ValueError,
     "tl.cnv_correlation: `profiles` has 9 windows, X_cnv has 10"),
    ("container width mismatch", {"profiles": _container(w=11)}, ValueError,
     "tl.cnv_correlation: `profiles` has 11 windows, X_cnv has 10"),
    ("container without the key", {"profiles": _container(key="X_other")}, KeyError,
     "tl.cnv_correlation: X_cnv not found in profiles.obsm. Did `tl.cnv_pseudobulk` make `profiles`?"),
    ("1-D profiles", {"profiles": np.zeros(10)}, ValueError, "tl.cnv_correlation: `profiles` must be 2-D (G x W), got 1-D"),
    ("NaN profile", {"profiles": NAN_PROFILE}, ValueError, "tl.cnv_correlation: `profiles` has non-finite values"),
    ("inf profile", {"profiles": np.where(np.isnan(NAN_PROFILE), np.inf, 1.0)}, ValueError,
     "tl.cnv_correlation: `profiles` has non-finite values"),
    ("missing groupby", {"groupby": "nope"}, KeyError, "tl.cnv_correlation: `nope` not found in `adata.obs`"),
    ("missing cnv_leiden", {"groupby": "cnv_leiden"}, KeyError,
     "tl.cnv_correlation: `cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?"),
    ("min_cells=0", {"groupby": "clone", "min_cells": 0}, ValueError,
     "tl.cnv_correlation: min_cells=0 must be an integer >= 1"),
]


@pytest.mark.parametrize("cid, kw, kind, message", BAD, ids=[c[0] for c in BAD])
def test_every_bad_argument_has_its_exception_and_its_whole_message(cid, kw, kind, message):
    import infercnvpy_amd as cnv

    ad = _adata()
    with pytest.raises(kind) as info:
        cnv.tl.cnv_correlation(ad, **kw)
    assert type(info.value) is kind and info.value.args[0] == message
    assert set(ad.obsm) == {"X_cnv"} and list(ad.obs.columns) == ["clone"] and set(ad.uns) == {"cnv"}


def test_bad_matrices_are_refused_by_both_functions():
    import infercnvpy_amd as cnv

    for fn, who in ((cnv.tl.cnv_correlation, "tl.cnv_correlation"), (cnv.tl.cnv_signal, "tl.cnv_signal")):
        with pytest.raises(ValueError) as info:
            fn(_adata(x=np.ones(6)))
        assert info.value.args[0] == f"{who}: X_cnv must be 2-D"
        with pytest.raises(ValueError) as info:
            fn(_adata(x=np.ones((6, 0))))
        assert info.value.args[0] == f"{who}: empty matrix of shape (6, 0)"
    with pytest.raises(KeyError) as info:
        cnv.tl.cnv_signal(_adata(), use_rep="other")
    assert info.value.args[0] == "tl.cnv_signal: X_other not found in adata.obsm. Did you run `tl.infercnv`?"

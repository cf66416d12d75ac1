"""GPU tests (``-m gpu``): tl.pca -- the float64 MFMA Gram (icv_gram_f64) against numpy, the whole call against the
fixtures recorded from sklearn and against the numpy oracle, host and HBM-resident X_cnv giving the same bits, and
the error paths."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import cases
from _pca_oracle import fixture_names, load_fixture, pca_oracle, ulp_tol, PCA_DIR

pytestmark = pytest.mark.gpu

BLOCK = 8192  # ICV_GRAM_BLOCK


def _gram_ref(x):
    xl = x.astype(np.longdouble)
    return (xl.T @ xl).astype(np.float64), np.abs(x).T @ np.abs(x)


def _check_gram(x, g):
    ref, bound = _gram_ref(x)
    assert np.all(np.abs(g - ref) <= 1e-12 * bound), float(np.max(np.abs(g - ref) - 1e-12 * bound))
    assert np.array_equal(g, g.T), "G is not bitwise symmetric"


def _values(n, w, seed, density=0.4, empty_rows=()):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, w)) * np.exp(rng.uniform(-3, 3, size=(1, w)))  # not float32-exact
    x[rng.uniform(size=(n, w)) > density] = 0
    x[list(empty_rows)] = 0
    return x


@pytest.mark.parametrize("w", [1, 3, 17, 1802, 2049])
@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_gram_small_n_matches_numpy(n, w):
    from infercnvpy_amd import _engine

    x = _values(n, w, seed=n * 7 + w, empty_rows=(0,) if n > 1 else ())
    for inp in (x, sp.csr_matrix(x)):
        g, s = _engine.gram(inp, zero_center=True)
        _check_gram(x, g)
        np.testing.assert_allclose(s, x.sum(axis=0), rtol=1e-13, atol=1e-300)


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 31, 2 * BLOCK + 33])
def test_gram_block_and_panel_boundaries(n, monkeypatch):
    import torch

    from infercnvpy_amd import _engine

    x = _values(n, 70, seed=n, density=0.3, empty_rows=range(0, n, 97))
    g1, _ = _engine.gram(sp.csr_matrix(x))
    _check_gram(x, g1)
    g2, _ = _engine.gram(sp.csr_matrix(x))
    assert np.array_equal(g1, g2), "two calls differ"
    g3, _ = _engine.gram(torch.from_numpy(x).cuda())  # dense rows, float64 panel
    assert np.array_equal(g1, g3)
    monkeypatch.setattr(_engine, "_gram_rows", lambda *a: BLOCK)  # one panel per block: the same bits
    g4, _ = _engine.gram(sp.csr_matrix(x))
    g5, _ = _engine.gram(x)
    assert np.array_equal(g1, g4) and np.array_equal(g1, g5)


def test_gram_float32_panel_is_exact_for_float32_values():
    from infercnvpy_amd import _engine

    x = _values(3000, 130, seed=5).astype(np.float32)
    g32, _ = _engine.gram(sp.csr_matrix(x))  # float32 panel
    g64, _ = _engine.gram(sp.csr_matrix(x.astype(np.float64)))  # float64 panel
    assert np.array_equal(g32, g64)
    _check_gram(x.astype(np.float64), g32)


def _fixture_input(f):
    import os

    return np.load(os.path.join(os.path.dirname(PCA_DIR), str(f["source"]) + ".npz"), allow_pickle=False)["out"]


@pytest.mark.parametrize("name", fixture_names())
def test_pca_matches_sklearn_fixtures(name):
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    f = load_fixture(name)
    x = _fixture_input(f)
    zc = bool(f["zero_center"])
    ad = SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32))
    ad.obsm["X_cnv"] = sp.csr_matrix(x)
    assert cnv.tl.pca(ad, zero_center=zc) is None
    got = ad.obsm["X_cnv_pca"]
    assert got.dtype == np.float32 and got.shape == (x.shape[0], int(f["n_comps"]))
    ref = f["x_pca"]
    sub = got[f["rows"]].astype(np.float64)
    tol = ulp_tol(ref)
    assert np.all(np.abs(sub - ref) <= tol), float(np.max(np.abs(sub - ref) / tol))
    big = np.abs(ref) > tol
    assert np.array_equal(np.sign(sub[big]), np.sign(ref[big]))

    # inplace=False, return_info, float64, dense input
    xp, comp, ratio, ev = cnv.tl.pca(ad, zero_center=zc, inplace=False, return_info=True, dtype="float64",
                                     use_rep="cnv", svd_solver="randomized", random_state=123)
    assert xp.dtype == np.float64
    np.testing.assert_allclose(comp[:, f["cols"]], f["components"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(ev, f["explained_variance"], rtol=1e-10)
    np.testing.assert_allclose(ratio, f["explained_variance_ratio"], rtol=1e-10)
    sv = np.sqrt(ev * (x.shape[0] - 1)) if zc else np.linalg.norm(xp, axis=0)
    np.testing.assert_allclose(sv, f["singular_values"], rtol=1e-10)
    assert np.array_equal(xp.astype(np.float32), got)
    ad.obsm["X_dense"] = x
    assert np.array_equal(cnv.tl.pca(ad, zero_center=zc, inplace=False, use_rep="dense"), got)


def _chain_inputs(n=5000, seed=3):
    v = cases.synthetic_var([4000, 3500, 3000, 2600, 2400, 2000, 1500, 1000], extra=(("chrX", 500), (None, 10)))
    X = cases.synthetic_expr(n, len(v["names"]), seed=seed)
    var = pd.DataFrame({"chromosome": v["chromosome"], "start": v["start"], "end": v["end"]}, index=v["names"])
    return X, var


def test_realistic_chain_host_and_resident():
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    X, var = _chain_inputs()
    assert X.shape[1] >= 20000
    ref = X[:500].mean(axis=0)
    ad = SimpleAnnData(X, var=var)
    cnv.tl.infercnv(ad, reference=ref)
    x_cnv = ad.obsm["X_cnv"]
    assert sp.issparse(x_cnv) and x_cnv.shape[1] > 1500
    for zc in (False, True):
        cnv.tl.pca(ad, zero_center=zc, key_added=f"pca{int(zc)}")
        exp, _, _, _ = pca_oracle(x_cnv, 50, zc)
        got = ad.obsm[f"X_pca{int(zc)}"]
        assert np.all(np.abs(got.astype(np.float64) - exp) <= ulp_tol(exp))

    adr = SimpleAnnData(torch.from_numpy(X).cuda(), var=var)
    cnv.tl.infercnv(adr, reference=ref)
    assert isinstance(adr.obsm["X_cnv"], cnv.PackedCsr)
    for zc in (False, True):
        cnv.tl.pca(adr, zero_center=zc, key_added=f"pca{int(zc)}")
        assert np.array_equal(adr.obsm[f"X_pca{int(zc)}"], ad.obsm[f"X_pca{int(zc)}"])


def test_zero_center_large_offset():
    import infercnvpy_amd as cnv

    rng = np.random.RandomState(4)
    x = rng.standard_normal((4000, 90)) * rng.uniform(0.5, 2.0, size=(1, 90))
    x += 10.0 * x.std(axis=0).max() * rng.uniform(0.5, 1.0, size=(1, 90))
    exp, comp_e, ratio_e, ev_e = pca_oracle(x, 20, True)
    got, comp, ratio, ev = cnv.tl.pca(_ad(x), zero_center=True, inplace=False, n_comps=20, return_info=True)
    assert np.all(np.abs(got.astype(np.float64) - exp) <= ulp_tol(exp))
    np.testing.assert_allclose(ev, ev_e, rtol=1e-10)
    np.testing.assert_allclose(comp, comp_e, rtol=0, atol=1e-10)


def _ad(x):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32))
    ad.obsm["X_cnv"] = x
    return ad


def test_error_paths():
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    x = _values(40, 12, seed=1)
    with pytest.raises(KeyError, match=r"X_cnv is not in adata.obsm. Did you run `tl.infercnv`\?"):
        cnv.tl.pca(SimpleAnnData(np.zeros((4, 2), dtype=np.float32)))
    with pytest.raises(ValueError):
        cnv.tl.pca(_ad(x), n_comps=12)
    with pytest.raises(ValueError):
        cnv.tl.pca(_ad(x[:1]))
    bad = x.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        cnv.tl.pca(_ad(sp.csr_matrix(bad)))
    with pytest.raises(TypeError, match="chunked"):
        cnv.tl.pca(_ad(x), chunked=True)
    assert cnv.tl.pca(_ad(x), inplace=False).shape == (40, 11)

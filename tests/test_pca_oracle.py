"""CPU tests: the numpy oracle of tl.pca (tests/_pca_oracle.py: float64 SVD, sklearn's sign rule, the cast) equals the
fixtures recorded from sklearn (tests/golden/make_pca_golden.py), and live sklearn where it is installed."""
import numpy as np
import pytest
import scipy.sparse as sp

from _pca_oracle import default_n_comps, fixture_names, load_fixture, pca_oracle, ulp_tol

NAMES = fixture_names()


def _input(f):
    import os

    from _pca_oracle import PCA_DIR

    return np.load(os.path.join(os.path.dirname(PCA_DIR), str(f["source"]) + ".npz"), allow_pickle=False)["out"]


def test_fixtures_present():
    assert len(NAMES) >= 10
    assert {bool(load_fixture(n)["zero_center"]) for n in NAMES} == {False, True}


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_fixture(name):
    f = load_fixture(name)
    x = _input(f)
    k = int(f["n_comps"])
    assert k == default_n_comps(*x.shape)
    xp, comp, ratio, ev = pca_oracle(x, k, bool(f["zero_center"]))
    got = xp[f["rows"]].astype(np.float64)
    assert np.all(np.abs(got - f["x_pca"]) <= ulp_tol(f["x_pca"]))
    big = np.abs(f["x_pca"]) > ulp_tol(f["x_pca"])
    assert np.array_equal(np.sign(got[big]), np.sign(f["x_pca"][big]))
    np.testing.assert_allclose(comp[:, f["cols"]], f["components"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(ev, f["explained_variance"], rtol=1e-10)
    np.testing.assert_allclose(ratio, f["explained_variance_ratio"], rtol=1e-10)


@pytest.mark.parametrize("zero_center", [False, True])
def test_oracle_matches_live_sklearn(zero_center):
    dec = pytest.importorskip("sklearn.decomposition")
    rng = np.random.RandomState(11)
    x = rng.gamma(0.3, 1.0, size=(300, 70))
    x[x < 0.5] = 0
    x += 3.0 * zero_center
    k = default_n_comps(*x.shape)
    if zero_center:
        est = dec.PCA(n_components=k, svd_solver="arpack", random_state=0)
        ref = est.fit_transform(x)
    else:
        est = dec.TruncatedSVD(n_components=k, algorithm="arpack", random_state=0)
        ref = est.fit_transform(sp.csr_matrix(x))
    xp, comp, ratio, ev = pca_oracle(x, k, zero_center)
    ref = ref.astype(np.float32).astype(np.float64)
    assert np.all(np.abs(xp.astype(np.float64) - ref) <= ulp_tol(ref))
    np.testing.assert_allclose(comp, est.components_, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ev, est.explained_variance_, rtol=1e-9)
    np.testing.assert_allclose(ratio, est.explained_variance_ratio_, rtol=1e-9)

"""CPU tests: the numpy oracle of tl.pca (tests/_pca_oracle.py: float64 SVD, sklearn's sign rule, the cast) equals the
fixtures recorded from sklearn (tests/golden/make_pca_golden.py), and live sklearn where it is installed; the oracles of
the two kernels (exact_fma / project_oracle, integer_matrix / int_gram) against independent arithmetic."""
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from _pca_oracle import (default_n_comps, exact_fma, fixture_names, int_gram, integer_matrix, load_fixture, muladd_chain,
                         pca_oracle, project_chain, project_oracle, projection_case, ulp_tol)

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


# ---- the oracles of icv_project and icv_gram_f64 -----------------------------------------------------------------------
def test_exact_fma_where_it_differs_from_multiply_add():
    a = 1.0 + 2.0 ** -30
    assert a * a - 1.0 == 2.0 ** -29  # the product is rounded first: 2^-60 is lost
    assert exact_fma(a, a, -1.0) == 2.0 ** -29 + 2.0 ** -60
    # a product that rounds to its addend's negative: multiply-add gives 0, the fma the rounding error of the product
    x, y = 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53
    p = x * y
    assert x * y - p == 0.0
    assert exact_fma(x, y, -p) == float(Fraction(x) * Fraction(y) - Fraction(p)) != 0.0
    # one rounding, to nearest even: an exact tie goes down to 1, anything above it goes up
    assert exact_fma(2.0 ** -53, 1.0, 1.0) == 1.0
    assert exact_fma(2.0 ** -53, 1.0 + 2.0 ** -52, 1.0) == 1.0 + 2.0 ** -52
    # (1 + 2^-27)^2 = 1 + 2^-26 + 2^-54 rounds to 1 + 2^-26; adding 2^-53 then makes a tie that goes to even, while
    # the exact sum 1 + 2^-26 + 2^-53 + 2^-54 lies above the tie
    b = 1.0 + 2.0 ** -27
    assert b * b + 2.0 ** -53 == 1.0 + 2.0 ** -26
    assert exact_fma(b, b, 2.0 ** -53) == 1.0 + 2.0 ** -26 + 2.0 ** -52


def test_exact_fma_where_it_agrees_with_multiply_add():
    rng = np.random.RandomState(2)
    for a, b, c in rng.randint(-2 ** 20, 2 ** 20, size=(200, 3)).astype(np.float64).tolist():
        assert exact_fma(a, b, c) == a * b + c  # small integers: nothing is rounded
    for a, b, c in ((0.0, 3.5, 0.0), (0.0, -3.5, 1.25), (1.5, 0.0, -2.0), (0.5, 0.25, 0.125), (3.0, 1.0 / 3.0, 0.0),
                    (1e300, 1e-300, 1.0), (2.0 ** -600, 2.0 ** -600, 0.0), (5e-324, 1.0, 5e-324)):
        assert exact_fma(a, b, c) == a * b + c, (a, b, c)
    assert isinstance(exact_fma(1.0, 2.0, 3.0), float)


def test_project_oracle_close_to_longdouble_and_unlike_multiply_add():
    x, v, shift = projection_case(9, 70, 33, seed=1)
    assert not x[1].any() and x[0].all() and 0.4 < np.count_nonzero(x[2:]) / x[2:].size < 0.6
    assert (x.astype(np.float32).astype(np.float64) != x)[x != 0].all()  # no value is a float32 number
    chain = project_chain(x, v)
    ref = (x.astype(np.longdouble) @ v.astype(np.longdouble))
    mag = np.abs(x) @ np.abs(v)
    if np.finfo(np.longdouble).eps < 2.0 ** -60:  # the bound of a chain of up to 70 roundings, each <= ulp(partial) / 2
        assert np.all(np.abs(chain - ref) <= 70 * 2.0 ** -53 * mag)
    got = project_oracle(x, v)
    assert got.dtype == np.float64 and np.array_equal(got, chain)
    assert np.array_equal(got[1], np.zeros(33))
    # CSR and dense give the same numbers; stored zeros and -0.0 are no-ops
    xs = sp.csr_matrix(x)
    assert np.array_equal(project_chain(xs[:4], v), chain[:4])
    xz = sp.csr_matrix((np.r_[xs.data[:5], 0.0, xs.data[6:]], xs.indices, xs.indptr), shape=xs.shape)
    xd = xz.toarray()
    xd[2, np.flatnonzero(xd[2] == 0)[0]] = -0.0
    assert xz.nnz == xs.nnz and np.array_equal(project_chain(xz[:3], v), project_chain(xd[:3], v))
    # the shift is one float64 subtraction after the chain, the cast comes last and once
    s64 = project_oracle(x, v, shift, chain=chain)
    assert np.array_equal(s64, chain - shift[None, :]) and np.array_equal(s64[1], -shift)
    s32 = project_oracle(x, v, shift, np.float32, chain=chain)
    assert s32.dtype == np.float32 and np.array_equal(s32, s64.astype(np.float32))
    assert np.array_equal(project_oracle(x[:3], v[:, :2], shift[:2], np.float32), s32[:3, :2])
    # an fma chain is not a multiply-add chain: the GPU test can tell the two contracts apart
    other = muladd_chain(x, v)
    n_diff = int(np.count_nonzero(other != chain))
    print(f"{n_diff} of {chain.size} results differ from the multiply-add chain")
    assert n_diff >= chain.size // 4
    assert np.all(np.abs(other - chain) <= 70 * 2.0 ** -52 * mag)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_integer_matrix_and_int_gram(dtype):
    x = integer_matrix(65, 129, seed=3, density=0.4, dtype=dtype)
    assert sp.isspmatrix_csr(x) and x.dtype == dtype and x.shape == (65, 129) and x.has_canonical_format
    assert np.array_equal(x.data, np.rint(x.data)) and x.data.min() == -7 and x.data.max() == 7 and (x.data != 0).all()
    assert 0.25 < x.nnz / (65 * 129) < 0.4
    d = x.toarray().astype(np.float64)
    g = int_gram(x)
    assert g.dtype == np.int64 and g.shape == (129, 129)
    assert np.array_equal(g, d.T @ d) and np.array_equal(g, g.T)
    assert np.array_equal(int_gram(x, dense=False).toarray(), g) and np.array_equal(int_gram(d), g)
    assert np.array_equal(integer_matrix(65, 129, seed=3, density=0.4, dtype=dtype).toarray(), x.toarray())
    with pytest.raises(AssertionError):
        integer_matrix(2 ** 20, 4, seed=0, density=0.1, hi=2 ** 17)
    with pytest.raises(AssertionError):
        int_gram(sp.csr_matrix(np.array([[0.5, 1.0]])))

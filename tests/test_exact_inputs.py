"""CPU checks of the exact-input generators (tests/_exact_inputs.py) that the bit-exact GPU tests of the Gram,
IQR selection and distance kernels rely on."""
import numpy as np
import pytest
from scipy.spatial.distance import pdist, squareform

import _exact_inputs as E
from oracle import infercnv_oracle as O


def _emulate_row_normalize(X):
    """float64 emulation of k_row_normalize (mean, centred squared norm, scale) on float32 rows."""
    x = X.astype(np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    return (d * (1.0 / np.sqrt((d * d).sum(axis=1, keepdims=True)))).astype(np.float32)


@pytest.mark.parametrize("n,k,p", [(2, 4, 1), (5, 15, 3), (16, 17, 16), (129, 143, 7), (130, 1802, 40),
                                   (9, 20000, 9)])
def test_corr_inputs_are_exact(n, k, p):
    X, labels, P, N = E.corr_case(n, k, p, seed=n + k)
    assert X.dtype == np.float32 and X.shape == (n, k)
    assert ((P != 0).sum(axis=1) == N).all() and (P.sum(axis=1) == 0).all()
    C = E.exact_corr(P, labels, N)
    z = _emulate_row_normalize(X)
    # z has entries 0 and +-2^-j exactly, and the float64 Gram of z is the exact matrix
    assert set(np.unique(np.abs(z))) <= {0.0, np.float32(1.0 / np.sqrt(N))}
    np.testing.assert_array_equal(z.astype(np.float64) @ z.astype(np.float64).T, C)
    # ... which agrees with numpy's corrcoef / the oracle's score up to corrcoef's own rounding
    np.testing.assert_allclose(np.corrcoef(X.astype(np.float64)), C, rtol=0, atol=1e-12)
    assert E.iqr(C) == pytest.approx(O.ith_score(X, ["g"] * n)["g"], abs=1e-12)
    np.testing.assert_array_equal(np.diag(C), 1.0)


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 16, 17, 100, 129, 130])
@pytest.mark.parametrize("p", [1, 2, 7])
def test_weighted_percentile_matches_numpy(n, p):
    """The weighted reference equals np.percentile of the materialised matrix, bit for bit (even and odd n)."""
    X, labels, P, N = E.corr_case(n, 17, p, seed=3 * n + p)
    C = E.exact_corr(P, labels, N)
    counts = np.bincount(labels, minlength=p)
    assert E.pattern_iqr(P, N, counts) == E.iqr(C)
    vals, w = np.unique(C, return_counts=True)
    assert E.weighted_percentile(vals, w, [75, 25]) == list(np.percentile(C, [75, 25]))


def test_weighted_percentile_random_values():
    rng = np.random.default_rng(0)
    for m in range(1, 60):
        v = rng.standard_normal(m)
        w = rng.integers(1, 4, m)
        flat = np.repeat(v, w)
        srt = np.sort(flat)
        for q in (0, 10, 25, 30, 50, 75, 99, 100):
            assert E.weighted_percentile(v, w, [q]) == [np.percentile(flat, q)]
            # shifted ranks: the values at floor(pos) + shift and the next rank, interpolated at the same weight
            pos = (srt.size - 1) * (q / 100.0)
            for shift in (-1, 1):
                r = min(max(int(np.floor(pos)) + shift, 0), srt.size - 1)
                exp = E.lerp(srt[r], srt[min(r + 1, srt.size - 1)], pos - np.floor(pos))
                assert E.weighted_percentile(v, w, [q], shift) == [exp]
    # values 0 .. 4, q = 30: the ranks 1, 2 moved to 2, 3 at weight 0.2
    assert E.weighted_percentile(np.arange(5.0), np.ones(5), [30], 1) == [2.2]


def test_tie_break_case_has_teeth():
    """The hand-built group moves with either rank and with the interpolation branch."""
    X, C = E.tie_break_case()
    z = _emulate_row_normalize(X)
    np.testing.assert_array_equal(np.clip(z.astype(np.float64) @ z.astype(np.float64).T, -1, 1), C)
    v = np.sort(C.ravel())
    m = v.size
    got = E.iqr(C)
    assert got == 0.125 + 2.0 ** -55

    def variant(shift=0, swap=False):
        qs = []
        for q in (0.75, 0.25):
            pos = (m - 1) * q
            r = int(np.floor(pos)) + shift
            a, b, t = v[r], v[min(r + 1, m - 1)], pos - np.floor(pos)
            d = b - a
            qs.append((a + d * t if t >= 0.5 else b - d * (1 - t)) if swap else E.lerp(a, b, t))
        return qs[0] - qs[1]

    assert variant() == got
    assert variant(shift=1) != got and variant(shift=-1) != got and variant(swap=True) != got


@pytest.mark.parametrize("n,k", [(8, 17), (1024, 288), (2048, 1802)])
def test_rank_boundary_case_has_teeth(n, k):
    """The constructed groups move when both ranks move by one either way, and the weighted reference with
    ``shift`` says by how much."""
    X, labels, P, N, counts = E.rank_boundary_case(n, k, seed=n)
    C = E.exact_corr(P, labels, N)
    got = E.iqr(C)
    assert E.pattern_iqr(P, N, counts) == got
    v = np.sort(C.ravel())
    m = v.size
    for shift in (1, -1):
        qs = []
        for q in (0.75, 0.25):
            pos = (m - 1) * q
            r = int(np.floor(pos)) + shift
            qs.append(E.lerp(v[r], v[min(r + 1, m - 1)], pos - np.floor(pos)))
        assert qs[0] - qs[1] == E.pattern_iqr(P, N, counts, shift) != got


@pytest.mark.parametrize("n,d,dup", [(1, 1, 0), (2, 1, 0), (3, 5, 0), (127, 16, 3), (128, 17, 5), (129, 143, 0),
                                     (1025, 288, 8)])
def test_distance_inputs_are_exact(n, d, dup):
    X, Zc = E.dist_case(n, d, seed=n, dup=dup)
    assert X.dtype == np.float32 and X.shape == (n, d)
    x = X.astype(np.float64)
    mean = x.sum(axis=0) / n
    np.testing.assert_array_equal(x - mean, Zc)  # the kernel's centring is exact
    assert (Zc.sum(axis=0) == 0).all()
    # every partial sum of the fp32 Gram is an integer below 2^24
    assert np.abs(Zc).max(initial=0) <= 7 and (np.abs(Zc) @ np.abs(Zc).T).max() < 2 ** 24
    D = E.exact_sqdist(Zc)
    assert D.dtype == np.int64
    np.testing.assert_array_equal(D, squareform(pdist(x, "sqeuclidean")) if n > 1 else np.zeros((1, 1)))
    np.testing.assert_array_equal(D, D.T)
    np.testing.assert_array_equal(np.diag(D), 0)
    if dup:
        assert (D[~np.eye(n, dtype=bool)] == 0).sum() >= 2 * dup
    rows = [0, n // 2, n - 1]
    np.testing.assert_array_equal(E.exact_sqdist(Zc, rows), D[rows])


def test_dyadic_cnv_sums_are_exact():
    x = E.dyadic_cnv(300, 77, seed=1)
    assert (x * 8 == np.round(x * 8)).all() and np.abs(x).max() <= 3
    s32 = np.abs(x).astype(np.float32).sum(axis=1, dtype=np.float32)
    np.testing.assert_array_equal(s32.astype(np.float64), np.abs(x).sum(axis=1))

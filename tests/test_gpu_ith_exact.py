"""Bit-exact tests of the correlation IQR (``icv_corr_iqr``: k_row_normalize, the fp32 MFMA Gram and the radix
selection of k_key_hist plus its host loop) on inputs where float32 makes no rounding error (tests/_exact_inputs.py):
the score must equal ``np.percentile(exact, [75, 25])`` of the exact correlation matrix with ``==``.

test_gpu_parity.py holds the same path to 1e-5 against float64 numpy; at that tolerance a percentile rank off by
one or a wrong interpolation branch goes unnoticed."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _exact_inputs as E

pytestmark = pytest.mark.gpu

NS = [2, 3, 4, 5, 8, 9, 16, 17, 128, 129, 130, 1024, 1025, 2001]
KS = [4, 15, 16, 17, 143, 160, 161, 288, 1802]


def _gpu(X):
    import torch

    return torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()


def _corr_iqr(X):
    from infercnvpy_amd import _engine

    return _engine.corr_iqr(_gpu(X))


def _adata(X_cnv, groups, X=None):
    from infercnvpy_amd._compat import SimpleAnnData

    n = len(groups)
    obs = pd.DataFrame({"group": pd.Categorical(groups)}, index=[f"c{i}" for i in range(n)])
    return SimpleAnnData(np.zeros((n, 1), dtype=np.float32) if X is None else X, obs=obs,
                         obsm={} if X_cnv is None else {"X_cnv": X_cnv})


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
def test_corr_iqr_exact(n, k):
    """Many patterns (all four targets distinct for most shapes): even n reach the t >= 0.5 branch of the
    interpolation, odd n^2 the scalar tail of the histogram's 16-byte loads; k on both sides of the 16-column LDS
    stage and of the 8-stage flush loop."""
    X, labels, P, N = E.corr_case(n, k, p=min(n, 48), seed=1000 * n + k)
    C = E.exact_corr(P, labels, N)
    assert _corr_iqr(X) == E.iqr(C)


@pytest.mark.parametrize("n,k", [(2, 4), (5, 17), (130, 161), (1025, 288), (2001, 1802)])
@pytest.mark.parametrize("p", [1, 2])
def test_corr_iqr_exact_shared_prefixes(n, k, p):
    """One pattern (every entry 1: IQR exactly 0) and two patterns: the four targets share their key prefixes."""
    X, labels, P, N = E.corr_case(n, k, p=p, seed=7 * n + p)
    C = E.exact_corr(P, labels, N)
    got = _corr_iqr(X)
    assert got == E.iqr(C)
    if p == 1:
        assert got == 0.0


def test_corr_iqr_tie_break_case():
    """A group whose IQR moves with either percentile rank and with numpy's interpolation branch."""
    X, C = E.tie_break_case()
    assert _corr_iqr(X) == E.iqr(C) == 0.125 + 2.0 ** -55


@pytest.mark.parametrize("n,k,pad", [(129, 143, 5), (1025, 288, 64), (17, 15, 1)])
def test_corr_iqr_exact_strided(n, k, pad):
    """A column slice of a wider tensor: row stride wider than k."""
    from infercnvpy_amd import _engine

    X, labels, P, N = E.corr_case(n, k, p=min(n, 30), seed=n + pad)
    wide = np.full((n, k + pad), 1e30, dtype=np.float32)
    wide[:, :k] = X
    xd = _gpu(wide)[:, :k]
    assert xd.stride(0) == k + pad
    assert _engine.corr_iqr(xd) == E.iqr(E.exact_corr(P, labels, N))


def test_corr_iqr_nan_rows():
    """A constant row gives NaN (numpy's 0/0), and so does a row holding inf, as in numpy."""
    X, labels, P, N = E.corr_case(40, 161, p=10, seed=3)
    for bad in ("const", "inf", "-inf"):
        Y = X.copy()
        if bad == "const":
            Y[7] = 2.5
        else:
            Y[7, 11] = np.inf if bad == "inf" else -np.inf
        with np.errstate(invalid="ignore", divide="ignore"):
            assert np.isnan(E.iqr(np.corrcoef(Y.astype(np.float64))))
        assert np.isnan(_corr_iqr(Y))
    assert _corr_iqr(X) == E.iqr(E.exact_corr(P, labels, N))  # and the next call is clean


@pytest.mark.parametrize("n,k", [(8, 17), (1024, 288), (2048, 1802)])
def test_corr_iqr_rank_boundary(n, k):
    """Groups where q25 sits on the edge of a run of equal correlations: a selection off by one rank is caught at
    large n too (elsewhere heavy ties hide it)."""
    X, labels, P, N, counts = E.rank_boundary_case(n, k, seed=n)
    exp = E.iqr(E.exact_corr(P, labels, N))
    assert E.pattern_iqr(P, N, counts, 1) != exp
    assert _corr_iqr(X) == exp


@pytest.mark.parametrize("n,counts", [
    (65537, (65537,)),         # one pattern: all 4 295 098 369 entries are 1.0, in one histogram bucket (> 2^32)
    (65537, (50000, 15537)),   # 2 741 395 369 entries equal 1.0: one bucket between 2^31 and 2^32
    (65537, (30001, 20000, 9000, 6000, 536)),  # five patterns
    (65540, None),             # q25 on the edge of a run of equal values
])
def test_corr_iqr_group_over_2_32_entries(n, counts):
    """Groups with more than 2^32 correlation entries, checked against the weighted reference (the matrix itself
    is 17.2 GB).  The ranks pass 2^31 (q75's are about 3.2e9), and in the first two cases one value fills a
    histogram bucket of k_key_hist past 2^32 and past 2^31 entries: a 32-bit counter, unsigned or signed, would
    lose them.  n = 65 537 gives an odd n^2, so the histogram's scalar tail runs."""
    import torch

    k, N = 64, 16
    free, _ = torch.cuda.mem_get_info()
    need = 24 << 30
    if free < need:
        pytest.skip(f"needs ~24 GB of free HBM for the {n} x {n} float32 matrix, {free / 2 ** 30:.1f} GB free")
    if counts is None:
        X, labels, P, N, counts = E.rank_boundary_case(n, k, seed=n, N=N)
        assert E.pattern_iqr(P, N, counts, 1) != E.pattern_iqr(P, N, counts)
    else:
        counts = np.asarray(counts)
        rng = np.random.default_rng(n + len(counts))
        P = E.corr_patterns(len(counts), k, N, rng)
        labels = rng.permutation(np.repeat(np.arange(len(counts)), counts))
        X = E.corr_cells(P, labels, rng)
    assert counts.sum() == n and n * n > 2 ** 32
    Pf = P.astype(np.float64)
    V = (Pf @ Pf.T) / N
    ones = int((np.outer(counts, counts) * (V == 1.0)).sum())
    if len(counts) == 1:
        assert ones == n * n > 2 ** 32
    elif len(counts) == 2:
        assert 2 ** 31 < ones < 2 ** 32 and V[0, 1] < 1.0
    exp = E.pattern_iqr(P, N, counts)
    got = _corr_iqr(X)
    assert got == exp
    assert (exp == 0.0) == (len(counts) == 1)


def _groups_case():
    """Four groups of X_cnv rows with offsets 0 (so a CSR stores only the pattern): a NaN group (all-zero rows)
    between two finite ones in the order the groups are scored, and a single cell."""
    rng = np.random.default_rng(11)
    k = 143
    N = E.support_size(k)
    sizes = {"A": 129, "C": 6, "D": 300, "B": 1}
    P = E.corr_patterns(25, k, N, rng)
    rows, groups, exp = [], [], {}
    for g, sz in sizes.items():
        lab = rng.integers(0, len(P), sz)
        X = E.corr_cells(P, lab, rng, offset=False)
        if g == "C":
            X[:] = 0.0  # all-zero rows: every correlation NaN
        rows.append(X)
        groups += [g] * sz
        if sz > 1:
            exp[g] = np.nan if g == "C" else E.iqr(E.exact_corr(P, lab, N))
    return np.vstack(rows), groups, exp


def _check(res, exp):
    assert set(res) == set(exp)
    for g, v in exp.items():
        if np.isnan(v):
            assert np.isnan(res[g]), g
        else:
            assert res[g] == v, (g, res[g], v)


def test_ithcna_exact_host_dense_and_device_inputs():
    """tl.ithcna on host CSR float64, dense float32 and a device PackedCsr of the same values."""
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    X, groups, exp = _groups_case()
    m = sp.csr_matrix(X.astype(np.float64))
    assert m.nnz == int((X != 0).sum())  # the zeros are not stored
    pk = _engine.PackedCsr(torch.from_numpy(m.indptr.astype(np.int64)).cuda(),
                           torch.from_numpy(m.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(m.data.astype(np.float64)).cuda(), m.shape[1])
    for x_cnv in (m, X, pk):
        ad = _adata(x_cnv, groups)
        _check(cnv.tl.ithcna(ad, "group", inplace=False), exp)
        if x_cnv is X:
            with pytest.raises(KeyError):  # the single-cell group, as the reference
                cnv.tl.ithcna(ad, "group")


def test_ithcna_exact_dense_with_offsets_and_scales():
    import infercnvpy_amd as cnv

    rng = np.random.default_rng(5)
    parts, groups, exp = [], [], {}
    for g, (n, k, p) in {"a": (64, 288, 9), "b": (300, 288, 2), "c": (17, 288, 17)}.items():
        X, labels, P, N = E.corr_case(n, k, p, seed=int(rng.integers(1 << 30)))
        parts.append(X)
        groups += [g] * n
        exp[g] = E.iqr(E.exact_corr(P, labels, N))
    X = np.vstack(parts)
    ad = _adata(X, groups)
    _check(cnv.tl.ithcna(ad, "group", inplace=False), exp)
    cnv.tl.ithcna(ad, "group")
    for g, v in exp.items():
        assert (ad.obs["ithcna"].values[np.asarray(groups) == g] == v).all()


def test_ithgex_exact_long_k():
    """tl.ithgex over 20 000 genes (N = 16 384 nonzeros per pattern): the long-K path of the Gram."""
    import infercnvpy_amd as cnv

    parts, groups, exp = [], [], {}
    for g, (n, p) in {"x": (130, 12), "y": (33, 33)}.items():
        X, labels, P, N = E.corr_case(n, 20000, p, seed=n)
        assert N == 16384
        parts.append(X)
        groups += [g] * n
        exp[g] = E.iqr(E.exact_corr(P, labels, N))
    ad = _adata(None, groups, X=np.vstack(parts))
    _check(cnv.tl.ithgex(ad, "group", inplace=False), exp)


# --------------------------------------------------------------------------------------------------------------- #
# tl.cnv_score: multiples of 1/8 with |x| <= 3, so every sum is exact and the score equals the oracle's
# --------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("categorical", [True, False])
def test_cnv_score_exact(categorical):
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine
    from infercnvpy_amd._compat import SimpleAnnData
    from oracle import infercnv_oracle as O

    n, k = 3001, 257
    x = E.dyadic_cnv(n, k, seed=4)
    rng = np.random.default_rng(2)
    labels = np.asarray(["t", "b", "myeloid", "x", "solo"], dtype=object)[rng.integers(0, 4, n)]
    labels[1234] = "solo"
    exp = O.cnv_score(x, labels)
    m = sp.csr_matrix(x)
    pk = _engine.PackedCsr(torch.from_numpy(m.indptr.astype(np.int64)).cuda(),
                           torch.from_numpy(m.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(m.data.astype(np.float64)).cuda(), k)
    col = pd.Categorical(labels) if categorical else labels
    for x_cnv in (m, x.astype(np.float32), pk):
        ad = SimpleAnnData(np.zeros((n, 1), dtype=np.float32), obs=pd.DataFrame({"grp": col}),
                           obsm={"X_cnv": x_cnv})
        got = cnv.tl.cnv_score(ad, "grp", inplace=False)
        assert list(got) == list(exp)
        for g in exp:
            assert got[g] == exp[g], (g, got[g], exp[g])
        cnv.tl.cnv_score(ad, "grp")
        np.testing.assert_array_equal(ad.obs["cnv_score"].values, np.array([exp[g] for g in labels]))

"""CPU tests of pp.neighbors: the numpy oracle (tests/_neighbors_oracle.py) against sklearn's brute-force search and
against its own definition, the public function's argument validation (no GPU is touched before it), and the new
symbols of the C ABI."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import _neighbors_oracle as O


@pytest.mark.parametrize("d", [1, 3, 50])
def test_oracle_neighbour_sets_match_sklearn_brute(d):
    from sklearn.neighbors import NearestNeighbors

    k = 15
    x = O.mixture(2000, d, seed=10 + d)
    assert len(np.unique(x, axis=0)) == len(x), "the input must be duplicate free"
    idx, _, d2 = O.knn(x, k + 1)  # k neighbours: the (k-1)-th and k-th distances decide which rows are compared
    x64 = x.astype(np.float64)
    nn = NearestNeighbors(n_neighbors=k, algorithm="brute").fit(x64)
    got = nn.kneighbors(x64, return_distance=False)  # k entries, the cell itself among them
    gap = (d2[:, k - 1] - d2[:, k - 2]) > 1e-9 * d2[:, k - 1]
    print(f"d={d}: rows excluded for a near-tie: {int((~gap).sum())} of {len(x)}")
    assert (~gap).mean() <= 0.01
    for i in np.flatnonzero(gap):
        assert set(got[i]) - {i} == set(idx[i, : k - 1]), i


def test_oracle_rows_are_sorted_by_distance_then_index():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 4, size=(300, 2)).astype(np.float32)  # masses of ties and duplicates
    idx, dist, d2 = O.knn(x, 20)
    assert not (idx == np.arange(300)[:, None]).any()
    for i in range(300):
        keys = list(zip(d2[i], idx[i]))
        assert keys == sorted(keys)
        full = O.sq_dists(x, np.array([i]))[0]
        full[i] = np.inf
        rest = np.setdiff1d(np.arange(300), np.append(idx[i], i))
        assert all((full[j], j) > keys[-1] for j in rest)
    assert np.array_equal(dist, np.sqrt(d2).astype(np.float32))


@pytest.mark.parametrize("k", [2, 15, 30])
def test_oracle_sigma_solves_the_equation(k):
    x = O.mixture(500, 10, seed=3)
    r = O.neighbors(x, k)
    delta = r["knn_distances"].astype(np.float64)
    s = np.exp(-np.maximum(delta - r["rho"][:, None], 0) / r["sigma"][:, None]).sum(axis=1)
    ok = ~r["floored"]
    assert ok.sum() > 400
    assert np.all(np.abs(s[ok] - np.log2(k)) < 1e-5 + 1e-12)
    assert np.all(r["rho"] == delta[:, 0])


def test_oracle_connectivities_are_symmetric_and_canonical():
    x = O.mixture(400, 5, seed=4)
    x[50:61] = x[50]  # a block of duplicates
    r = O.neighbors(x, 8)
    c, dm = r["connectivities"], r["distances"]
    assert c.dtype == np.float32 and c.has_canonical_format
    assert (abs(c - c.T)).nnz == 0
    assert np.all(c.data > 0) and np.all(c.data <= 1)
    assert dm.dtype == np.float32 and np.all(np.diff(dm.indptr) == 7)
    assert np.all(np.diff(dm.indices.reshape(400, 7), axis=1) > 0)
    assert (dm.data == 0).sum() >= 11 * 7  # explicit zeros between the duplicates are stored


def test_oracle_five_points_by_hand():
    # points on a line at 0, 1, 3, 7, 7 (the last two duplicated), k = 3: two neighbours each
    x = np.array([[0.0], [1.0], [3.0], [7.0], [7.0]], dtype=np.float32)
    r = O.neighbors(x, 3)
    assert r["knn_indices"].tolist() == [[1, 2], [0, 2], [1, 0], [4, 2], [3, 2]]
    assert r["knn_distances"].tolist() == [[1, 3], [1, 2], [2, 3], [0, 4], [0, 4]]
    assert r["rho"].tolist() == [1, 1, 2, 4, 4]
    # rows 0..2: 1 + exp(-g / sigma) = log2(3) with g = 2, 1, 1; rows 3, 4: delta - rho = (-4, 0): both terms are 1,
    # the sum 2 > log2(3) for every sigma, so the bisection halves 64 times and the floor 1e-3 * mean(0, 4) applies
    e = np.log2(3.0) - 1.0
    assert np.allclose(r["sigma"][:3], [-2 / np.log(e), -1 / np.log(e), -1 / np.log(e)], rtol=1e-4)
    assert r["sigma"][3:].tolist() == [2e-3, 2e-3] and r["floored"].tolist() == [False] * 3 + [True] * 2
    w = r["weights"]
    assert np.allclose(w[:3], [[1, e], [1, e], [1, e]], atol=2e-5) and w[3:].tolist() == [[1, 1], [1, 1]]
    c = r["connectivities"].toarray().astype(np.float64)
    # A: 0->(1:1, 2:e) 1->(0:1, 2:e) 2->(1:1, 0:e) 3->(4:1, 2:1) 4->(3:1, 2:1)
    exp = np.zeros((5, 5))
    exp[0, 1] = exp[1, 0] = 1
    exp[0, 2] = exp[2, 0] = 2 * e - e * e
    exp[1, 2] = exp[2, 1] = 1  # e + 1 - e
    exp[3, 4] = exp[4, 3] = 1
    exp[2, 3] = exp[3, 2] = exp[2, 4] = exp[4, 2] = 1
    assert np.allclose(c, exp, atol=3e-5)
    assert r["distances"].toarray().tolist() == [[0, 1, 3, 0, 0], [1, 0, 2, 0, 0], [3, 2, 0, 0, 0], [0, 0, 4, 0, 0],
                                                 [0, 0, 4, 0, 0]]
    assert r["distances"].nnz == 10


# ---- the edge inputs of tests/test_gpu_neighbors_edges.py: the property that makes each one an edge ---------------------
TINY = float(np.finfo(np.float32).tiny)  # 2^-126


def test_hub_row_has_every_other_cell():
    c = O.neighbors(O.hub(), 15)["connectivities"]
    assert np.diff(c.indptr)[0] == 3000 - 1


def test_small_clusters_have_far_neighbours_of_weight_zero():
    x = O.small_clusters()
    r = O.neighbors(x, 15)
    same = r["knn_indices"] // 10 == np.arange(600)[:, None] // 10
    assert np.all(same[:, :9]) and not same[:, 9:].any()  # 9 near, 5 very far
    assert np.all(r["knn_distances"][:, :9] < 10) and np.all(r["knn_distances"][:, 9:] > 1e4)
    w32 = r["weights"].astype(np.float32)
    assert np.all(w32[:, 9:] == 0) and (w32 == 0).sum() == 3000 and w32.size == 8400
    assert np.all(np.diff(r["connectivities"].indptr) == 9)  # fewer than k - 1
    assert r["floored"].sum() == 600


def test_simplex_is_all_ties_and_floored():
    x = O.simplex()
    assert x.dtype == np.float32 and x.shape == (64, 64)
    r = O.neighbors(x, 15)
    full = O.sq_dists(x, np.arange(64))
    assert np.all(full[~np.eye(64, dtype=bool)] == 2.0)
    assert r["knn_indices"][5].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14]
    for i in range(64):  # every neighbour is a tie: the lowest indices win
        assert r["knn_indices"][i].tolist() == [j for j in range(16) if j != i][:14]
    assert np.all(r["rho"] > 0) and r["floored"].all()
    assert np.all(r["sigma"] == 1e-3 * r["rho"])  # the bisection halved 64 times to 2^-64, far below the floor


def test_near_duplicates_are_distinct_below_the_float32_keys():
    x = O.near_duplicates()
    assert x.dtype == np.float32 and x.shape == (3000, 50)
    diff = x[2001:2070] != x[2000]
    assert np.all(diff.sum(axis=1) == 1)  # one column each
    idx, dist, d2 = O.knn(x, 15)
    assert np.all((idx[2000] > 2000) & (idx[2000] < 2070))
    assert np.all(dist[2000] > 0) and np.all(dist[2000] < 1e-8) and np.all(d2[2000] < 1e-16)
    assert len(np.unique(dist[2000])) >= 4
    assert len(np.unique(d2[2000])) < 14  # exact ties
    assert float((x[2000].astype(np.float64) ** 2).sum()) > 1  # float32 keys of order 1: ulp 1e-7 >> d2


@pytest.mark.parametrize("p", [60, 100, -70, -100, -120])
def test_scaling_by_a_power_of_two_keeps_the_neighbours(p):
    x = O.mixture(1000, 50, seed=1)
    idx0, dist0, _ = O.knn(x, 15)
    xs = O.scaled(x, p)
    assert xs.dtype == np.float32 and np.isfinite(xs).all()
    idx, dist, _ = O.knn(xs, 15)
    assert np.array_equal(idx, idx0)
    n_sub = int(((xs != 0) & (np.abs(xs) < TINY)).sum())
    if p == -120:
        assert n_sub > 0  # (455 here)
        assert np.all(dist >= TINY) and dist.max() < 1e-35  # the distances stay normal numbers
    else:
        assert n_sub == 0 and np.array_equal(xs.astype(np.float64), x.astype(np.float64) * 2.0**p)
        assert np.array_equal(dist.astype(np.float64), dist0.astype(np.float64) * 2.0**p)
    z2 = ((xs.astype(np.float64) - xs.astype(np.float64).mean(axis=0)) ** 2).sum(axis=1)
    assert (z2.max() >= 1e37) == (p > 0)  # on which side of the sweep's magnitude gate (1e36) the input lies, with room
    assert (z2.min() > float(np.finfo(np.float32).max)) == (p == 100)  # |z|^2 overflows float32 on every row


def test_ladder_weights_pass_through_the_subnormals_to_zero():
    x = O.ladder()
    r = O.neighbors(x, O.LADDER_K)
    w = r["weights"]
    w32 = w.astype(np.float32)
    assert ((w32 > 0) & (w32 < TINY)).sum() >= 5  # (62 here)
    assert ((w32 == 0) & (w > 0)).sum() >= 5  # (96 here)
    # no weight within a factor e^(+-1e-6) of the round-to-zero boundary 2^-150 (nor any w == 0 in float64)
    assert np.all(w > 0) and np.abs(np.log(w) - 150 * np.log(0.5)).min() > 1e-6
    assert not (r["knn_indices"][12:] < 12).any()  # the rungs do not list the cluster: C = w there
    c = r["connectivities"]
    assert (c.data < TINY).sum() >= 5  # subnormal stored entries
    assert c[:12, 12:].nnz == ((w32[:12] != 0) & (r["knn_indices"][:12] >= 12)).sum() <= 12 * 18 - 5  # dropped ones


# ---- the public function without a GPU --------------------------------------------------------------------------------
def _adata(x, key="X_cnv_pca"):
    from infercnvpy_amd._compat import SimpleAnnData

    return SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32), obsm={key: x})


def test_public_interface_exists():
    import inspect

    import infercnvpy_amd

    sig = inspect.signature(infercnvpy_amd.pp.neighbors)
    assert list(sig.parameters)[:4] == ["adata", "use_rep", "key_added", "inplace"]
    assert sig.parameters["use_rep"].default == "cnv_pca" and sig.parameters["key_added"].default == "cnv_neighbors"
    assert sig.parameters["n_neighbors"].default == 15 and sig.parameters["inplace"].default is True
    from infercnvpy_amd._compat import SimpleAnnData

    assert SimpleAnnData(np.zeros((2, 2))).obsp == {}
    assert SimpleAnnData(np.zeros((2, 2)), obsp={"a": 1}).obsp == {"a": 1}


def test_argument_validation_needs_no_gpu():
    import infercnvpy_amd as cnv

    x = O.mixture(20, 4, seed=1)
    bad = x.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinity"):
        cnv.pp.neighbors(_adata(bad))
    bad[3, 1] = np.inf
    with pytest.raises(ValueError, match="NaN or infinity"):
        cnv.pp.neighbors(_adata(bad))
    with pytest.raises(ValueError, match="NaN or infinity"):  # finite in float64, infinite as float32
        cnv.pp.neighbors(_adata(x.astype(np.float64) * 1e38))
    for k in (1, 0, -3, 21, 65):
        with pytest.raises(ValueError, match="n_neighbors"):
            cnv.pp.neighbors(_adata(x), n_neighbors=k)
    with pytest.raises(ValueError, match="n_neighbors"):
        cnv.pp.neighbors(_adata(O.mixture(100, 4)), n_neighbors=65)
    with pytest.raises(ValueError, match="metric"):
        cnv.pp.neighbors(_adata(x), metric="cosine")
    with pytest.raises(ValueError, match="method"):
        cnv.pp.neighbors(_adata(x), method="gauss")
    with pytest.raises(ValueError, match="knn"):
        cnv.pp.neighbors(_adata(x), knn=False)
    with pytest.raises(ValueError, match="columns"):
        cnv.pp.neighbors(_adata(np.zeros((300, 257), dtype=np.float32)))
    with pytest.raises(ValueError, match="columns"):
        cnv.pp.neighbors(_adata(np.zeros((30, 0), dtype=np.float32)))
    with pytest.raises(KeyError, match="X_other"):
        cnv.pp.neighbors(_adata(x), use_rep="other")


def test_missing_cnv_pca_warns_and_runs_tl_pca(monkeypatch):
    import infercnvpy_amd as cnv

    called = []

    def fake_pca(adata, *a, **kw):
        called.append((a, kw))
        adata.obsm["X_cnv_pca"] = np.full((5, 2), np.nan, dtype=np.float32)  # stops at the validation, before the GPU

    monkeypatch.setattr(cnv.tl, "pca", fake_pca)
    ad = _adata(np.zeros((5, 2), dtype=np.float32), key="X_cnv")
    with pytest.warns(UserWarning, match="X_cnv_pca not found in adata.obsm. Computing PCA with default parameters"):
        with pytest.raises(ValueError, match="NaN or infinity"):
            cnv.pp.neighbors(ad)
    assert called == [((), {})]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        with pytest.raises(ValueError, match="NaN or infinity"):  # present now: no warning, no second PCA
            cnv.pp.neighbors(ad)
    assert len(called) == 1


KNN_SYMBOLS = ("icv_knn_workspace", "icv_knn", "icv_knn_fuzzy", "icv_knn_symmetrize_count", "icv_knn_symmetrize_fill",
               "icv_knn_sort_rows")


def test_knn_symbols_are_exported_and_declared():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "infercnv_hip.h")).read()
    for name in KNN_SYMBOLS:
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
        assert f"int {name}(" in header, name


def test_knn_workspace_is_linear_in_n_and_validates():
    from infercnvpy_amd import _lib

    lib = _lib.load()

    def ws(n, d, k):
        b = ctypes.c_int64(-1)
        rc = lib.icv_knn_workspace(n, d, k, ctypes.byref(b))
        return rc, b.value

    for n, d, k in ((1, 5, 2), (10, 0, 2), (10, 257, 2), (10, 5, 1), (10, 5, 11), (100, 5, 65)):
        assert ws(n, d, k)[0] == _lib.ICV_ERR_INVALID, (n, d, k)
    rc, b1 = ws(1 << 20, 50, 15)
    rc2, b16 = ws(1 << 24, 50, 15)
    assert rc == rc2 == _lib.ICV_OK
    per_cell = b16 / (1 << 24)
    assert abs(b1 / (1 << 20) - per_cell) < 1 and per_cell < 4 * 64 + 4 + 8 * 22 + 8 + 4 + 8  # header: bytes per cell

"""GPU tests (``-m gpu``): pp.neighbors against the numpy oracle of DESIGN.md 4.9 (tests/_neighbors_oracle.py).
Neighbour indices and distances are compared for EQUALITY (rule 2 / 3 leave no tolerance to choose), rho too, sigma
on the rows with rho > 0; the connectivities within one float32 ulp (two exp implementations)."""
import numpy as np
import pytest

import _neighbors_oracle as O

pytestmark = pytest.mark.gpu

NS = [2, 15, 16, 17, 63, 64, 65, 1000, 5001]
DS = [1, 2, 49, 50, 64, 65, 256]
KS = [2, 15, 30, 64]


def _adata(x, key="X_cnv_pca"):
    from infercnvpy_amd._compat import SimpleAnnData

    return SimpleAnnData(np.zeros((x.shape[0], 1), dtype=np.float32), obsm={key: x})


def _run(x, k):
    import infercnvpy_amd as cnv

    return cnv.pp.neighbors(_adata(x), n_neighbors=k, inplace=False, return_info=True)


def _check(x, k, got=None, what=""):
    n = x.shape[0]
    dist, conn, idx, kd, rho, sigma = got if got is not None else _run(x, k)
    exp = O.neighbors(x, k)
    assert idx.dtype == np.int32 and idx.shape == (n, k - 1) and kd.dtype == np.float32 and kd.shape == (n, k - 1)
    assert rho.dtype == np.float64 and rho.shape == (n,) and sigma.dtype == np.float64 and sigma.shape == (n,)
    bad = np.flatnonzero((idx != exp["knn_indices"]).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: {idx[bad[:1]]} vs {exp['knn_indices'][bad[:1]]}"
    assert np.array_equal(kd, exp["knn_distances"]), what
    assert np.array_equal(rho, exp["rho"]), what
    pos = exp["rho"] > 0
    assert np.array_equal(sigma[pos], exp["sigma"][pos]), what
    tol = n * k * 2.0**-53
    assert np.all(np.abs(sigma[~pos] - exp["sigma"][~pos]) <= tol * exp["sigma"][~pos]), what
    for m in (dist, conn):
        assert m.format == "csr" and m.shape == (n, n) and m.dtype == np.float32
    e = exp["distances"]
    assert np.array_equal(dist.indptr, e.indptr) and np.array_equal(dist.indices, e.indices), what
    assert np.array_equal(dist.data, e.data), what
    e = exp["connectivities"]
    assert np.array_equal(conn.indptr, e.indptr) and np.array_equal(conn.indices, e.indices), what
    assert np.all(np.abs(conn.data.astype(np.float64) - e.data) <= 2.0**-23 * np.abs(e.data.astype(np.float64))), what
    assert conn.has_canonical_format and np.all(conn.data != 0)
    t = conn.T.tocsr()
    t.sort_indices()
    assert np.array_equal(t.indptr, conn.indptr) and np.array_equal(t.indices, conn.indices)
    assert np.array_equal(t.data, conn.data), f"{what}: connectivities not bitwise symmetric"


@pytest.mark.parametrize("n", NS)
def test_sizes_dimensions_and_k(n):
    for d in DS:
        x = O.mixture(n, d, seed=1000 * d + n)
        for k in KS:
            if k <= n:
                _check(x, k, what=f"n={n} d={d} k={k}")


@pytest.mark.parametrize("n,d,k", [(1000, 50, 15), (5001, 50, 30), (1000, 3, 64)])
def test_large_common_offset(n, d, k):
    x = O.mixture(n, d, seed=7, offset=100.0)
    assert abs(x[:, 0].mean()) > 90 * x[:, 0].std() and abs(x[:, -1].mean()) > 90 * x[:, -1].std()
    _check(x, k, what="offset")


@pytest.mark.parametrize("n,d,k", [(64, 5, 15), (1000, 50, 15), (5001, 2, 30)])
def test_all_points_equal(n, d, k):
    x = np.full((n, d), 1.25, dtype=np.float32)
    _check(x, k, what="all equal")


@pytest.mark.parametrize("k", [2, 15, 64])
def test_duplicate_blocks(k):
    x = O.mixture(3000, 50, seed=11)
    x[100:111] = x[100]        # 11 copies
    x[2000:2070] = x[2000]     # 70 copies: more than k
    x[[5, 900, 2999]] = x[5]   # scattered copies
    _check(x, k, what="duplicates")


@pytest.mark.parametrize("side,k", [(32, 15), (71, 30)])
def test_regular_grid_ties_go_to_the_lower_index(side, k):
    g = np.arange(side, dtype=np.float32)
    x = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    _check(x, k, what="grid")


def test_forty_thousand_cells_and_the_fallback_is_rare():
    import torch

    from infercnvpy_amd import _engine

    n, k = 40000, 15
    x = O.mixture(n, 50, seed=5)
    idx, dist, n_exact = _engine.knn(torch.from_numpy(x).cuda(), k)
    print(f"rows sent to the exact kernel: {n_exact} of {n}")
    e_idx, e_dist, _ = O.knn(x, k)
    assert np.array_equal(idx.cpu().numpy(), e_idx)
    assert np.array_equal(dist.cpu().numpy(), e_dist)
    assert n_exact < 0.01 * n
    _check(x, k, what="40000")


def test_inplace_writes_what_scanpy_writes():
    import infercnvpy_amd as cnv

    x = O.mixture(300, 20, seed=2)
    ad = _adata(x, key="X_rep")
    assert cnv.pp.neighbors(ad, use_rep="rep", key_added="nb", n_neighbors=10, random_state=7) is None
    assert set(ad.obsp) == {"nb_distances", "nb_connectivities"}
    assert ad.uns["nb"] == {"connectivities_key": "nb_connectivities", "distances_key": "nb_distances",
                            "params": {"n_neighbors": 10, "method": "umap", "random_state": 7, "metric": "euclidean",
                                       "use_rep": "X_rep"}}
    out = cnv.pp.neighbors(ad, use_rep="rep", n_neighbors=10, inplace=False)
    assert len(out) == 2 and "cnv_neighbors" not in ad.uns
    for a, b in zip(out, (ad.obsp["nb_distances"], ad.obsp["nb_connectivities"])):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert np.array_equal(a.data, b.data)
    info = cnv.pp.neighbors(ad, use_rep="rep", n_neighbors=10, return_info=True)
    assert len(info) == 6 and "cnv_neighbors_distances" in ad.obsp
    _check(x, 10, got=info, what="inplace")


def _same(a, b):
    for u, v in zip(a, b):
        if hasattr(u, "indptr"):
            assert np.array_equal(u.indptr, v.indptr) and np.array_equal(u.indices, v.indices)
            assert np.array_equal(u.data, v.data)
        else:
            assert np.array_equal(u, v)


def test_same_bits_host_tensor_repeat_and_float64():
    import torch

    x = O.mixture(4097, 50, seed=3)
    first = _run(x, 15)
    _same(first, _run(x, 15))
    _same(first, _run(torch.from_numpy(x).cuda(), 15))
    x64 = x.astype(np.float64) * (1 + 2.0**-30)  # not float32 numbers; rounds back to x
    assert np.array_equal(x64.astype(np.float32), x) and not np.array_equal(x64, x)
    _same(first, _run(x64, 15))
    _same(first, _run(torch.from_numpy(x64).cuda(), 15))
    xi = np.round(x * 4).astype(np.int64)
    _same(_run(xi, 15), _run(xi.astype(np.float32), 15))


def test_chain_infercnv_pca_neighbors_on_golden():
    import pandas as pd

    import infercnvpy_amd as cnv
    from _golden import GoldenCase
    from infercnvpy_amd._compat import SimpleAnnData

    g = GoldenCase("big20k_w100_s10")
    var = pd.DataFrame({"chromosome": g.chromosome, "start": g.start, "end": g.start + 1},
                       index=[f"g{i}" for i in range(len(g.start))])
    ad = SimpleAnnData(g.X, var=var)
    cnv.tl.infercnv(ad, **g.api_kwargs())
    with pytest.warns(UserWarning, match="X_cnv_pca not found"):
        info = cnv.pp.neighbors(ad, return_info=True)
    x_pca = ad.obsm["X_cnv_pca"]
    assert x_pca.dtype == np.float32 and x_pca.shape == (g.X.shape[0], 50)
    assert ad.uns["cnv_neighbors"]["params"]["use_rep"] == "X_cnv_pca"
    _check(x_pca, 15, got=info, what="golden chain")

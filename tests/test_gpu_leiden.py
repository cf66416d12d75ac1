"""tl.leiden on the GPU: the labels equal the numpy oracle of DESIGN.md 4.10 bit for bit; the Leiden guarantees at sizes
where the oracle is too slow; the same bits for every input form; the chain up to tl.ithcna on a golden."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _leiden_oracle as lo  # noqa: E402
import _neighbors_oracle as no  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leiden", "louvain_q.npz")
GAMMAS = (0.5, 1.0, 2.0)
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = lo.mixture_graph(int(name[3:]), 0) if name.startswith("mix") else lo.small_graphs()[name]
    return _cache[name]


def _run(g, **kw):
    import infercnvpy_amd as cnv

    cat, info = cnv.tl.leiden(None, adjacency=g, inplace=False, return_info=True, **kw)
    assert list(cat.categories) == [str(i) for i in range(info["n_communities"])]
    return np.asarray(cat.codes, dtype=np.int32), info


NAMES = tuple(lo.small_graphs()) + ("mix2000", "mix5000")


@pytest.mark.parametrize("name", NAMES)
def test_labels_equal_the_oracle(name):
    g = _graph(name)
    for gamma in GAMMAS:
        for rs in (0, 1):
            for nit in (1, 2, -1):
                for uw in (True, False):
                    got, info = _run(g, resolution=gamma, random_state=rs, n_iterations=nit, use_weights=uw)
                    ref, rinfo = lo.leiden(g, gamma, rs, nit, uw, return_info=True)
                    what = (name, gamma, rs, nit, uw)
                    assert np.array_equal(got, ref), what
                    for key in ("levels", "rounds", "n_iterations", "bound_reached", "quality"):
                        assert info[key] == rinfo[key], (what, key)


@pytest.mark.parametrize("name", ("hub70000", "mix2000_hub", "cliques600"))
def test_long_rows_equal_the_oracle(name):
    """Rows beyond what the wavefront kernel stages in LDS (512 entries) take the workgroup-per-row kernel: a star of
    70 000 leaves, a mixture with a hub joined to every cell, cliques of 600 (299 < 512 < 599 entries per row)."""
    g = {"hub70000": lambda: lo.star(70_000), "mix2000_hub": lambda: lo.with_hub(_graph("mix2000")),
         "cliques600": lambda: lo.cliques([600, 300, 600], ring=True)}[name]()
    for gamma, rs, nit in ((1.0, 0, -1), (0.5, 1, 2), (2.0, 0, 1)):
        got, info = _run(g, resolution=gamma, random_state=rs, n_iterations=nit)
        ref, rinfo = lo.leiden(g, gamma, rs, nit, True, return_info=True)
        assert np.array_equal(got, ref), (name, gamma, rs, nit)
        for key in ("levels", "rounds", "n_iterations", "bound_reached", "quality"):
            assert info[key] == rinfo[key], (name, gamma, key)


def test_malformed_device_csr_is_a_value_error():
    import torch

    g = _graph("mix2000")
    indptr = torch.from_numpy(g.indptr.astype(np.int64)).cuda()
    indices = torch.from_numpy(g.indices.astype(np.int32)).cuda()
    data = torch.from_numpy(g.data).cuda()
    for bad in (indptr + 1, indptr * 2, torch.flip(indptr, (0,))):
        with pytest.raises(ValueError, match="indptr"):
            _run((bad, indices, data))


def _device_neighbors(n, d, seed):
    """pp.neighbors' connectivities of a mixture, as device CSR tensors."""
    import torch

    from infercnvpy_amd import _engine

    x = torch.from_numpy(no.mixture(n, d, seed)).cuda()
    idx, dist, _ = _engine.knn(x, 15)
    _, _, w = _engine.knn_fuzzy(dist, 15)
    return _engine.knn_symmetrize(idx, w, 15)


@pytest.mark.parametrize("n", (40_000, 200_000))
def test_guarantees_at_scale(n):
    indptr, indices, data = _device_neighbors(n, 10, 0)
    g = sp.csr_matrix((data.cpu().numpy(), indices.cpu().numpy(), indptr.cpu().numpy()), shape=(n, n))
    labels, info = _run((indptr, indices, data))
    print(f"n={n}: {info['n_communities']} communities, Q={info['quality']}, levels={info['levels'][0]}")
    lo.check_partition(labels)
    gi = lo.int_graph(g)
    lo.check_connected(gi, labels)
    assert not info["bound_reached"], info
    lo.check_node_optimal(gi, labels, 1.0)


def test_quality_against_louvain_golden():
    import make_leiden_golden as mg

    gold = np.load(GOLDEN)
    g = _graph("mix5000").astype(np.float64).tocsr()
    for gamma in GAMMAS:
        labels, _ = _run(g, resolution=gamma)
        ours = lo.modularity(g, labels, gamma)
        q = gold[mg.key(5000, gamma)]
        print(f"gamma={gamma}: Q={ours:.6f} Louvain Q in [{q.min():.6f}, {q.max():.6f}]")
        assert ours >= q.min() - (q.max() - q.min()), (gamma, ours, q.min(), q.max())


def test_same_bits_for_every_input_form():
    import torch

    import infercnvpy_amd as cnv

    g = _graph("mix2000")
    first, info = _run(g)
    for other in (g.tocsc(), g.tocoo(), g.astype(np.float64), sp.csr_matrix(g)):
        got, oinfo = _run(other)
        assert np.array_equal(first, got) and info == oinfo
    dev = (torch.from_numpy(g.indptr.astype(np.int64)).cuda(), torch.from_numpy(g.indices.astype(np.int32)).cuda(),
           torch.from_numpy(g.data).cuda())
    assert np.array_equal(first, _run(dev)[0])
    x = torch.from_numpy(no.mixture(3000, 20, 1)).cuda()  # other kernels use the pool in between
    cnv._engine.knn(x, 15)
    torch.cuda.synchronize()
    assert np.array_equal(first, _run(g)[0])
    g64 = g.astype(np.float64) * (1 + 2.0 ** -30)  # not float32 numbers; rounds back to g
    assert np.array_equal(first, _run(g64)[0])


def test_device_validation_errors():
    g = lo.wide_weights()
    bad = g.tolil()
    bad[0, 0] = 1.0
    for m, what in ((bad.tocsr(), "diagonal"), (sp.triu(g).tocsr(), "symmetric"), (-g, "negative"),
                    (g * np.inf, "finite"), (g * 2.0 ** 40, "too large")):
        with pytest.raises(ValueError, match=what):
            _run(m)


def test_inplace_writes_obs_and_uns_only():
    import pandas as pd

    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    g = _graph("mix2000")
    ad = SimpleAnnData(np.zeros((2000, 3), dtype=np.float32), obsp={"conn": g.copy()},
                       uns={"cnv_neighbors": {"connectivities_key": "conn"}})
    assert cnv.tl.leiden(ad, resolution=0.5, random_state=3, n_iterations=2) is None
    col = ad.obs["cnv_leiden"]
    assert isinstance(col.dtype, pd.CategoricalDtype)
    assert list(col.cat.categories) == [str(i) for i in range(len(col.cat.categories))]
    assert np.array_equal(col.cat.codes.to_numpy(), lo.leiden(g, 0.5, 3, 2))
    assert ad.uns["cnv_leiden"] == {"params": {"resolution": 0.5, "random_state": 3, "n_iterations": 2}}
    assert set(ad.obsp) == {"conn"} and (ad.obsp["conn"] != g).nnz == 0
    out = cnv.tl.leiden(ad, obsp="conn", key_added="other", inplace=False, resolution=0.5, random_state=3, n_iterations=2)
    assert "other" not in ad.obs and np.array_equal(np.asarray(out.codes), col.cat.codes.to_numpy())


def test_chain_up_to_ithcna_on_golden():
    import pandas as pd

    import infercnvpy_amd as cnv
    from _golden import GoldenCase
    from infercnvpy_amd._compat import SimpleAnnData

    g = GoldenCase("big20k_w100_s10")
    var = pd.DataFrame({"chromosome": g.chromosome, "start": g.start, "end": g.start + 1},
                       index=[f"g{i}" for i in range(len(g.start))])
    ad = SimpleAnnData(g.X, var=var)
    cnv.tl.infercnv(ad, **g.api_kwargs())
    cnv.tl.pca(ad)
    cnv.pp.neighbors(ad)
    cnv.tl.leiden(ad)
    col = ad.obs["cnv_leiden"]
    assert isinstance(col.dtype, pd.CategoricalDtype) and 1 <= len(col.cat.categories) < g.X.shape[0]
    lo.check_partition(col.cat.codes.to_numpy())
    lo.check_connected(lo.int_graph(ad.obsp["cnv_neighbors_connectivities"]), col.cat.codes.to_numpy())
    real_factorize = pd.factorize
    pd.factorize = None  # the categorical-codes path of cnv_score does not factorize
    try:
        cnv.tl.cnv_score(ad)
    finally:
        pd.factorize = real_factorize
    cnv.tl.ithcna(ad, "cnv_leiden")  # no default groupby: the reference's signature has none either
    assert np.isfinite(np.asarray(ad.obs["cnv_score"], dtype=np.float64)).all()
    assert len(ad.obs["ithcna"]) == g.X.shape[0]
    per_group = pd.Series(np.asarray(ad.obs["cnv_score"])).groupby(col.cat.codes.to_numpy()).nunique()
    assert (per_group == 1).all()  # one score per cluster: cnv_score grouped by what tl.leiden wrote

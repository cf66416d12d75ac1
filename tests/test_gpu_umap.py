"""tl.umap on the GPU: one epoch equals the numpy oracle of DESIGN.md 4.11 up to the last bit of pow; full runs are
compared GPU against GPU bit for bit and with the oracle's full run by neighbour preservation."""
import os
import sys
import time
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _leiden_oracle as lo  # noqa: E402
import _neighbors_oracle as no  # noqa: E402
import _umap_oracle as uo  # noqa: E402
from _umap_checks import check_epoch as _check_epoch  # noqa: E402
from _umap_checks import coincident as _coincident  # noqa: E402
from _umap_checks import device as _device  # noqa: E402
from _umap_checks import gpu_epochs as _gpu_epochs  # noqa: E402

pytestmark = pytest.mark.gpu
A, B = uo.A_DEFAULT, uo.B_DEFAULT
SETTINGS = ((2, 0), (3, 1))  # (n_components, random_state)
# Above this many entry activations the numpy oracle needs more than a few seconds for the trajectory up to epoch t
# (mix2000 up to t = 499: 6.4e6, 4.5 s); the snapshot of epoch t then comes from the device's own epochs [0, t), and
# the ONE epoch that is compared still runs on both sides from that same snapshot.
ORACLE_BUDGET = 8_000_000
# neighbour preservation (k = 14) of the ORACLE's full run on mix2000 (random init, 500 epochs, seeds 0-4), measured on
# the CPU: 0.29793, 0.29829, 0.29929, 0.29907, 0.29711
ORACLE_PRESERVATION_MIN, ORACLE_PRESERVATION_SPREAD = 0.29711, 0.00218
_cache = {}


def _mix(n):
    key = ("nb", n)
    if key not in _cache:
        _cache[key] = no.neighbors(no.mixture(n, 10, 0), 15)
    return _cache[key]


def _graph(name):
    if name not in _cache:
        small = lo.small_graphs()
        if name in small:
            g = small[name]
        elif name == "mix2000":
            g = _mix(2000)["connectivities"]
        elif name == "mix2000_hub":
            g = lo.with_hub(_mix(2000)["connectivities"])
        elif name == "isolated_vertex":  # vertex 300 has no entry
            g = sp.block_diag([lo.mixture_graph(300, 1), sp.csr_matrix((1, 1))]).tocsr()
        elif name == "n7":  # so few vertices that the negative samples hit k == i
            g = lo.cliques([4, 3], ring=True)
        elif name == "star70000":
            g = lo.star(70_000)
        _cache[name] = (g, uo.Graph(g))
    return _cache[name]


def _activations(og, t, n_epochs):
    e = np.flatnonzero(og.fires(n_epochs))
    return int(np.floor((t - 1) / (og.w_max / og.w[e])).sum()) if t > 1 and len(e) else 0


def _snapshots(name, dev, n_epochs, c, seed, epochs):
    """t -> the positions before epoch t: the oracle's own, from the random start."""
    og = _graph(name)[1]
    y0 = uo.random_init(og.n, c, seed)
    cheap = [t for t in epochs if _activations(og, t, n_epochs) <= ORACLE_BUDGET]
    last, snaps = uo.run(og, y0, 0, max(cheap), keep=cheap, n_epochs=n_epochs, a=A, b=B, seed=seed)
    snaps[max(cheap)] = last
    for t in epochs:
        if t not in snaps:
            snaps[t] = _gpu_epochs(dev, y0, 0, t, n_epochs, seed)
    return snaps


NAMES = tuple(lo.small_graphs()) + ("mix2000", "isolated_vertex", "mix2000_hub", "n7")


@pytest.mark.parametrize("n_epochs", (500, 30))
@pytest.mark.parametrize("name", NAMES)
def test_one_epoch_equals_the_oracle(name, n_epochs):
    g, og = _graph(name)
    dev = _device(g)
    epochs = (0, 1, 2, n_epochs // 2, n_epochs - 1)
    for c, seed in SETTINGS:
        snaps = _snapshots(name, dev, n_epochs, c, seed, epochs)
        for t in epochs:
            _check_epoch(og, dev, snaps[t], t, n_epochs, seed, (name, n_epochs, c, seed, t))
        for t in (0, 2, n_epochs // 2):
            _check_epoch(og, dev, _coincident(og, snaps[t]), t, n_epochs, seed, (name, n_epochs, c, seed, t, "d2 == 0"))


def test_one_epoch_of_a_row_of_70000_entries_equals_the_oracle():
    g, og = _graph("star70000")
    dev = _device(g)
    for c, seed in SETTINGS:
        snaps = _snapshots("star70000", dev, 200, c, seed, (1, 199))
        for t in (1, 199):
            _check_epoch(og, dev, snaps[t], t, 200, seed, ("star70000", c, seed, t))


def test_other_parameters_equal_the_oracle():
    """gamma, negative_sample_rate (0 as well), alpha and (a, b) reach the kernel as the oracle reads them."""
    import torch

    from infercnvpy_amd import _engine

    g, og = _graph("mix2000")
    dev = _device(g)
    y = uo.random_init(og.n, 2, 3) * np.float32(0.3)
    for kw in (dict(gamma=0.5, negative_sample_rate=3, initial_alpha=0.25), dict(negative_sample_rate=0),
               dict(gamma=0.0, negative_sample_rate=8)):
        ref, m = uo.epoch(og, y, 7, n_epochs=100, a=1.577, b=0.895, seed=3, **kw)
        yd = torch.from_numpy(y).cuda()
        _engine.umap_epochs(*dev, yd, a=1.577, b=0.895, n_epochs=100, epoch_begin=7, epoch_end=8, random_state=3, **kw)
        tol = np.spacing(np.abs(ref)).astype(np.float64) + m[:, None] * 2.0 ** -32
        assert (np.abs(yd.cpu().numpy().astype(np.float64) - ref) <= tol).all(), kw


def test_no_hidden_state():
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    g, og = _graph("mix2000")
    dev = _device(g)
    y0 = uo.random_init(og.n, 2, 0)
    whole = _gpu_epochs(dev, y0, 0, 40, 500, 0)
    y = y0
    for t in range(40):
        y = _gpu_epochs(dev, y, t, t + 1, 500, 0)
    assert whole.tobytes() == y.tobytes()
    assert not np.array_equal(whole, y0)

    kw = dict(inplace=False, init_pos="random", random_state=1)
    first = cnv.tl.umap(None, adjacency=g, **kw)
    assert first.dtype == np.float32 and first.shape == (og.n, 2)
    assert cnv.tl.umap(None, adjacency=g, **kw).tobytes() == first.tobytes()
    assert cnv.tl.umap(None, adjacency=dev, **kw).tobytes() == first.tobytes()
    assert cnv.tl.umap(None, adjacency=g.tocoo().astype(np.float64), **kw).tobytes() == first.tobytes()
    ad = SimpleAnnData(np.zeros((og.n, 3), dtype=np.float32), obsp={"conn": g.copy()})
    assert cnv.tl.umap(ad, obsp="conn", **kw).tobytes() == first.tobytes()
    assert "X_cnv_umap" not in ad.obsm
    ad.uns["cnv_neighbors"] = {"connectivities_key": "conn"}
    assert cnv.tl.umap(ad, init_pos="random", random_state=1) is None
    assert ad.obsm["X_cnv_umap"].tobytes() == first.tobytes()
    assert ad.uns["cnv_umap"]["params"] == {"a": pytest.approx(A, abs=1e-6), "b": pytest.approx(B, abs=1e-6),
                                            "random_state": 1}
    ad.obsm["start"] = y0
    import torch

    for init in ("start", y0, torch.from_numpy(y0).cuda()):
        got = cnv.tl.umap(ad, init_pos=init, maxiter=40, a=A, b=B, inplace=False)
        assert got.tobytes() == _gpu_epochs(dev, y0, 0, 40, 40, 0).tobytes()


def test_full_run_quality():
    """The oracle's own full runs (ORACLE_PRESERVATION_*: min 0.29711, max - min 0.00218 over seeds 0-4) set the bar:
    the device's value must reach the oracle's minimum minus that spread."""
    import infercnvpy_amd as cnv

    nb = _mix(2000)
    g = nb["connectivities"]
    bound = ORACLE_PRESERVATION_MIN - ORACLE_PRESERVATION_SPREAD
    for seed in (0, 1, 2):
        y, info = cnv.tl.umap(None, adjacency=g, inplace=False, init_pos="random", random_state=seed, return_info=True)
        p = uo.neighbour_preservation(nb["knn_indices"], y, 14)
        print(f"seed {seed}: preservation {p:.5f} (bound {bound:.5f}), max |y| {np.abs(y).max():.2f}, {info['stage_ms']}")
        assert info["n_epochs"] == 500 and info["n_fire"] == int(uo.Graph(g).fires(500).sum())
        assert np.isfinite(y).all() and np.abs(y).max() < 50
        assert p >= bound, (seed, p)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="tl.umap")  # no fall-back to the random start here
        y, info = cnv.tl.umap(None, adjacency=g, inplace=False, return_info=True)  # the spectral default
        again = cnv.tl.umap(None, adjacency=g, inplace=False)
    assert info["init_pos"] == "spectral" and y.tobytes() == again.tobytes()
    p = uo.neighbour_preservation(nb["knn_indices"], y, 14)
    print(f"spectral: preservation {p:.5f}")
    assert np.isfinite(y).all() and np.abs(y).max() < 50 and p >= bound


def test_two_components_warn_and_fall_back_to_random():
    import infercnvpy_amd as cnv

    g = lo.cliques([40, 30])
    with pytest.warns(UserWarning, match="connected component"):
        y, info = cnv.tl.umap(None, adjacency=g, inplace=False, return_info=True, maxiter=50)
    assert info["init_pos"] == "random"
    assert y.tobytes() == cnv.tl.umap(None, adjacency=g, inplace=False, init_pos="random", maxiter=50).tobytes()


def test_device_validation_errors():
    import torch

    import infercnvpy_amd as cnv

    g = lo.wide_weights()
    bad = g.tolil()
    bad[0, 0] = 1.0
    for m, what in ((bad.tocsr(), "diagonal"), (sp.triu(g).tocsr(), "symmetric"), (-g, "negative"), (g * np.inf, "finite")):
        with pytest.raises(ValueError, match=what):
            cnv.tl.umap(None, adjacency=m, inplace=False, init_pos="random")
    indptr, indices, data = _device(g)
    for wrong in (indptr + 1, indptr * 2, torch.flip(indptr, (0,))):
        with pytest.raises(ValueError, match="indptr"):
            cnv.tl.umap(None, adjacency=(wrong, indices, data), inplace=False, init_pos="random")


def test_scale_200000_cells():
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    n = 200_000
    x = torch.from_numpy(no.mixture(n, 10, 0)).cuda()
    idx, dist, _ = _engine.knn(x, 15)
    _, _, w = _engine.knn_fuzzy(dist, 15)
    dev = _engine.knn_symmetrize(idx, w, 15)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y, info = cnv.tl.umap(None, adjacency=dev, inplace=False, init_pos="random", return_info=True)
    wall = time.perf_counter() - t0
    again = cnv.tl.umap(None, adjacency=dev, inplace=False, init_pos="random")
    assert info["n_epochs"] == 200 and np.isfinite(y).all() and y.tobytes() == again.tobytes()
    knn_idx = idx.cpu().numpy()
    k = knn_idx.shape[1]
    rows = np.random.default_rng(0).choice(n, 2000, replace=False)
    p = uo.neighbour_preservation(knn_idx, y, k, rows=rows, block=64)
    print(f"n={n}: wall {wall:.3f} s, {info['stage_ms']}, nnz {dev[1].numel()}, fire {info['n_fire']}, "
          f"preservation {p:.4f} (chance {k / n:.6f}), max |y| {np.abs(y).max():.1f}")
    assert p >= 10 * k / n


def test_chain_up_to_pl_umap_on_golden():
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
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
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # so few cells may well give a disconnected graph: the random start then
        cnv.tl.umap(ad)
    n = g.X.shape[0]
    assert ad.obsm["X_cnv_umap"].shape == (n, 2) and np.isfinite(ad.obsm["X_cnv_umap"]).all()
    ax = cnv.pl.umap(ad, color="cnv_leiden")
    try:
        assert len(ax.collections[0].get_offsets()) == n
        assert ax.get_legend() is not None
    finally:
        plt.close(ax.figure)

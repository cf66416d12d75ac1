"""tl.tsne on the GPU: an iteration, and a whole run, equal the numpy oracle of DESIGN.md 4.12 bit for bit; the affinities
equal it too (beta and W); full runs are judged by neighbour preservation against sklearn's."""
import os
import sys
import time

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _leiden_oracle as lo  # noqa: E402
import _neighbors_oracle as no  # noqa: E402
import _tsne_oracle as to  # noqa: E402
import _umap_oracle as uo  # noqa: E402

pytestmark = pytest.mark.gpu
TILE = 256  # kTsTile of csrc/icv_tsne.hpp
# neighbour preservation (k = 14) and max |y| of sklearn 1.7.2's TSNE(perplexity=30, early_exaggeration=12,
# learning_rate=1000, init="random") on no.mixture(2000, 10, 0), seeds 0-4, measured on the CPU:
#   barnes_hut SK2000_BH, exact SK2000_EXACT
SK2000_BH = (0.42946, 0.43125, 0.42750, 0.42854, 0.42829)
SK2000_EXACT = (0.42668, 0.42521, 0.43004, 0.42996, 0.43036)
SK2000_MAX_ABS = 81.68  # the largest max |y| of those ten layouts
SK2000_MIN = min(SK2000_BH + SK2000_EXACT)
SK2000_SPREAD = max(SK2000_BH + SK2000_EXACT) - SK2000_MIN
_cache = {}


def _mix(n):
    if ("x", n) not in _cache:
        _cache["x", n] = no.mixture(n, 10, 0)
    return _cache["x", n]


def _tsne_graph(x, perplexity=30.0):
    """The oracle's W of the points x."""
    kk = to.n_neighbors(len(x), perplexity)
    idx, dist, _ = no.knn(x, kk + 1)
    _, p = to.affinities(dist, perplexity)
    return to.symmetrize(idx, p)


def _scaled(g):
    """A test graph with its values brought into the range of affinities (W <= 2)."""
    g = sp.csr_matrix(g).astype(np.float64)
    return g * (1.0 / g.max()) if g.nnz else g


def _graph(name):
    if name not in _cache:
        if name == "mix2000":
            g = _tsne_graph(_mix(2000))
        elif name == "mix300":
            g = _tsne_graph(_mix(300))
        elif name == "mix2000_hub":
            g = lo.with_hub(_tsne_graph(_mix(2000)))
        elif name == "isolated_vertex":  # vertex 300 has no entry
            g = sp.block_diag([_tsne_graph(_mix(300)), sp.csr_matrix((1, 1))]).tocsr()
        elif name == "n2":
            g = lo.path(2)
        elif name == "n3":
            g = lo.path(3)
        elif name == "n7":
            g = _scaled(lo.cliques([4, 3], ring=True))
        elif name == "n65":
            g = _tsne_graph(_mix(65), 10.0)
        elif name == "tile_plus_1":
            g = _tsne_graph(_mix(TILE + 1), 10.0)
        elif name == "star5000":
            g = lo.star(4999)
        _cache[name] = (g, to.Graph(g))
    return _cache[name]


def _device(g):
    import torch

    g = sp.csr_matrix(g)
    g.sort_indices()
    return (torch.from_numpy(g.indptr.astype(np.int64)).cuda(), torch.from_numpy(g.indices.astype(np.int32)).cuda(),
            torch.from_numpy(g.data.astype(np.float32)).cuda())


def _gpu(dev, state, t0, t1, **kw):
    import torch

    from infercnvpy_amd import _engine

    y, u, gain = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in state)
    _engine.tsne_iterations(*dev, y, u, gain, iter_begin=t0, iter_end=t1, **kw)
    return y.cpu().numpy(), u.cpu().numpy(), gain.cpu().numpy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _positions(n, c, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "1e-4":
        return to.random_init(n, c, seed)
    if kind in ("1", "1e3"):
        return (rng.normal(size=(n, c)) * float(kind)).astype(np.float32)
    y = rng.normal(size=(n, c)).astype(np.float32)
    if kind == "duplicated":  # every third cell sits on the cell before it
        y[2::3] = y[1:-1:3][:len(y[2::3])]
        return y
    assert kind == "coincident"
    y[:] = y[0]
    return y


ITERS = (0, 1, 249, 250, 251, 999)
SMALL = ("n2", "n3", "n7", "n65", "tile_plus_1", "isolated_vertex")
LARGE = ("mix2000", "mix2000_hub", "star5000")


def _check_iteration(og, dev, state, t, what):
    ref = to.iteration(og, *state, t)
    got = _gpu(dev, state, t, t + 1)
    for name, r, g in zip(("y", "u", "gain"), ref, got):
        assert g.tobytes() == r.tobytes(), (what, name, int((g != r).sum()), float(np.abs(g - r).max()))
    return ref


@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("name", SMALL)
def test_one_iteration_equals_the_oracle_small(name, c):
    """Every iteration of ITERS from the oracle's own state (the trajectory is cheap: the state before iteration t is
    taken from a run of the oracle with the schedule moved, which changes no rule), for every kind of position."""
    g, og = _graph(name)
    dev = _device(g)
    for kind in ("1e-4", "1", "1e3", "duplicated", "coincident"):
        state = to.start(_positions(og.n, c, kind, 1))
        # three oracle iterations give a state with non-trivial updates and gains
        state = to.run(og, state, 0, 3)
        if kind == "coincident":
            assert state[0].tobytes() == to.start(_positions(og.n, c, kind, 1))[0].tobytes()  # gradient exactly 0
        for t in ITERS:
            _check_iteration(og, dev, state, t, (name, c, kind, t))
    # and along the device's own trajectory from the small random start
    state = to.start(to.random_init(og.n, c, 0))
    for t in (0, 1):
        state = _check_iteration(og, dev, state, t, (name, c, "trajectory", t))


@pytest.mark.parametrize("c", (2, 3))
@pytest.mark.parametrize("name", LARGE)
def test_one_iteration_equals_the_oracle_large(name, c):
    """The oracle is O(n^2) per iteration: the state before iteration t comes from the device's own iterations [0, t),
    and the ONE iteration that is compared runs on both sides from that same state."""
    g, og = _graph(name)
    dev = _device(g)
    # the oracle needs 1.2 s per iteration of the 5 000-cell star: fewer iterations and kinds of positions there
    iters, kinds = ((0, 250), ("1e3", "duplicated")) if name == "star5000" else (ITERS, ("1", "1e3", "duplicated", "coincident"))
    start = to.start(to.random_init(og.n, c, c))
    for t in iters:
        state = _gpu(dev, start, 0, t) if t else start
        assert all(np.isfinite(a).all() for a in state)
        _check_iteration(og, dev, state, t, (name, c, t))
    for kind in kinds:
        state = to.start(_positions(og.n, c, kind, 2))
        ref = _check_iteration(og, dev, state, 0, (name, c, kind))
        if kind == "coincident":
            assert ref[0].tobytes() == state[0].tobytes()


def test_no_hidden_state():
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    g, og = _graph("mix300")
    dev = _device(g)
    start = to.start(to.random_init(og.n, 2, 0))
    whole = _gpu(dev, start, 0, 60, exaggeration_iters=30)
    state = start
    for t in range(60):
        state = _gpu(dev, state, t, t + 1, exaggeration_iters=30)
    assert _same(whole, state) and not np.array_equal(whole[0], start[0])
    assert not _same(whole, _gpu(dev, start, 0, 60))  # the switch at 30 did something

    x = _mix(300)
    kw = dict(inplace=False, max_iter=60)
    first = cnv.tl.tsne(None, use_rep=x, **kw)
    assert first.dtype == np.float32 and first.shape == (300, 2)
    assert cnv.tl.tsne(None, use_rep=x, **kw).tobytes() == first.tobytes()
    assert cnv.tl.tsne(None, use_rep=torch.from_numpy(x).cuda(), **kw).tobytes() == first.tobytes()
    assert cnv.tl.tsne(None, use_rep=x.astype(np.float64), **kw).tobytes() == first.tobytes()
    ad = SimpleAnnData(np.zeros((300, 3), dtype=np.float32), obsm={"X_cnv_pca": x.copy(), "X_dev": torch.from_numpy(x).cuda()})
    assert cnv.tl.tsne(ad, **kw).tobytes() == first.tobytes()
    assert cnv.tl.tsne(ad, use_rep="dev", **kw).tobytes() == first.tobytes()
    assert "X_cnv_tsne" not in ad.obsm and "cnv_tsne" not in ad.uns
    assert cnv.tl.tsne(ad, max_iter=60) is None
    assert ad.obsm["X_cnv_tsne"].tobytes() == first.tobytes()
    assert ad.uns["cnv_tsne"]["params"] == {"perplexity": 30, "early_exaggeration": 12, "learning_rate": 1000,
                                            "random_state": 0, "use_rep": "X_cnv_pca"}
    y, info = cnv.tl.tsne(ad, key_added="other", max_iter=60, return_info=True, init_pos="random", random_state=3)
    assert ad.obsm["X_other"] is y and ad.uns["other"]["params"]["random_state"] == 3
    assert info["n_neighbors_used"] == 63 and info["n_iter"] == 60 and info["init_pos"] == "random"
    assert set(info["stage_ms"]) == {"knn_ms", "affinities_ms", "symmetrise_ms", "validation_ms", "iterations_ms"}
    assert y.tobytes() != first.tobytes()
    assert cnv.tl.tsne(ad, n_pcs=5, **kw).tobytes() == cnv.tl.tsne(None, use_rep=x[:, :5], **kw).tobytes()
    # given positions: as a key, an array, a tensor
    y0 = to.random_init(300, 2, 7)
    ad.obsm["start"] = y0
    ref = _gpu(_device(_tsne_graph(x)), to.start(y0), 0, 60)[0]
    for init in ("start", y0, torch.from_numpy(y0).cuda()):
        got, info = cnv.tl.tsne(ad, init_pos=init, return_info=True, **kw)
        assert got.tobytes() == ref.tobytes() and info["init_pos"] == "given"


def test_whole_run_equals_the_oracle():
    """100 iterations on the 300-cell mixture, from the points to the layout: every stage on the device."""
    import infercnvpy_amd as cnv

    x = _mix(300)
    for c, init in ((2, "pca"), (3, "random")):
        ref, _ = to.tsne(x, n_components=c, max_iter=100, init_pos=init, random_state=5)
        got = cnv.tl.tsne(None, use_rep=x, inplace=False, n_components=c, max_iter=100, init_pos=init, random_state=5)
        assert got.tobytes() == ref.tobytes(), (c, init, int((got != ref).sum()))
    assert np.isfinite(ref).all() and np.abs(ref).max() > 1e-2  # it moved


def _duplicated_rows():
    x = _mix(500).copy()
    x[100:180] = x[100]   # 80 equal rows: all 63 distances are 0
    x[200:210] = x[200]   # 10 equal rows: 9 zeros, then ordinary distances
    return x


@pytest.mark.parametrize("case", ("mix500", "mix2000", "duplicated"))
def test_affinities_equal_the_oracle(case):
    import torch

    from infercnvpy_amd import _engine

    x = {"mix500": lambda: _mix(500), "mix2000": lambda: _mix(2000), "duplicated": _duplicated_rows}[case]()
    for perplexity in (30.0, 5.0):
        kk = to.n_neighbors(len(x), perplexity)
        idx, dist, _ = no.knn(x, kk + 1)
        beta, p = to.affinities(dist, perplexity)
        w = to.symmetrize(idx, p)
        d_idx, d_dist, _ = _engine.knn(torch.from_numpy(x).cuda(), kk + 1)
        assert np.array_equal(d_idx.cpu().numpy(), idx) and np.array_equal(d_dist.cpu().numpy(), dist)
        d_beta, d_cond = _engine.tsne_affinities(d_dist, perplexity)
        d_beta = d_beta.cpu().numpy()
        bad = np.flatnonzero(d_beta != beta)
        assert bad.size == 0, (case, perplexity, bad[:5], d_beta[bad[:5]], beta[bad[:5]])
        indptr, indices, data = (t.cpu().numpy() for t in _engine.tsne_symmetrize(d_idx, d_cond))
        assert np.array_equal(indptr, w.indptr) and np.array_equal(indices, w.indices), (case, perplexity)
        # knn_sym_value<true> rounds the float64 sum p_ij + p_ji to float32 once, as the oracle does: equal, not close
        assert data.dtype == np.float32 and data.tobytes() == w.data.tobytes(), (case, perplexity, int((data != w.data).sum()))
        if case == "duplicated":
            assert (beta[100:180] == 1.0).all() and np.array_equal(p[100:180], np.full((80, kk), 1.0 / kk))


def test_full_run_quality():
    """sklearn's own runs (SK2000_*) set the bar: preservation >= their minimum minus their spread, max |y| below twice
    the largest of theirs (the exact repulsion and the truncated neighbourhood change the scale a little, not its
    order)."""
    import infercnvpy_amd as cnv

    x = _mix(2000)
    knn_idx, _, _ = no.knn(x, 15)
    bound = SK2000_MIN - SK2000_SPREAD
    for kw in (dict(init_pos="random", random_state=0), dict(init_pos="random", random_state=1),
               dict(init_pos="random", random_state=2), dict()):
        t0 = time.perf_counter()
        y, info = cnv.tl.tsne(None, use_rep=x, inplace=False, return_info=True, **kw)
        wall = time.perf_counter() - t0
        p = uo.neighbour_preservation(knn_idx, y, 14)
        print(f"{kw}: preservation {p:.5f} (bound {bound:.5f}), max |y| {np.abs(y).max():.2f}, wall {wall:.3f} s, "
              f"{info['stage_ms']}")
        assert info["n_iter"] == 1000 and info["n_neighbors_used"] == 63
        assert info["init_pos"] == kw.get("init_pos", "pca")
        assert np.isfinite(y).all() and np.abs(y).max() < 2 * SK2000_MAX_ABS
        assert p >= bound, (kw, p)


def test_scale_20000_cells():
    import torch

    import infercnvpy_amd as cnv

    n = 20_000
    x = torch.from_numpy(no.mixture(n, 10, 0)).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y, info = cnv.tl.tsne(None, use_rep=x, inplace=False, return_info=True)
    wall = time.perf_counter() - t0
    again = cnv.tl.tsne(None, use_rep=x, inplace=False)
    assert info["n_iter"] == 1000 and np.isfinite(y).all() and y.tobytes() == again.tobytes()
    from infercnvpy_amd import _engine

    knn_idx = _engine.knn(x, 15)[0].cpu().numpy()
    rows = np.random.default_rng(0).choice(n, 2000, replace=False)
    p = uo.neighbour_preservation(knn_idx, y, 14, rows=rows, block=64)
    print(f"n={n}: wall {wall:.3f} s, {info['stage_ms']}, preservation {p:.4f} (chance {14 / n:.6f}), "
          f"max |y| {np.abs(y).max():.1f}")
    assert p >= 10 * 14 / n


def test_errors():
    import torch

    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    x = _mix(300)
    kw = dict(inplace=False, max_iter=1)
    with pytest.raises(ValueError, match="perplexity"):
        cnv.tl.tsne(None, use_rep=x, perplexity=63, **kw)
    with pytest.raises(ValueError, match="perplexity"):
        cnv.tl.tsne(None, use_rep=x[:20], perplexity=19, **kw)
    with pytest.raises(ValueError, match="random_state"):
        cnv.tl.tsne(None, use_rep=x, random_state=0.5, **kw)
    for c in (1, 4, 2.5, "2", True):
        with pytest.raises(ValueError, match="n_components"):
            cnv.tl.tsne(None, use_rep=x, n_components=c, **kw)
    with pytest.raises(ValueError, match="unsupported keyword.*method"):
        cnv.tl.tsne(None, use_rep=x, method="barnes_hut", **kw)
    with pytest.raises(ValueError, match="non-finite"):
        cnv.tl.tsne(None, use_rep=x, init_pos=np.full((300, 2), np.nan), **kw)
    with pytest.raises(ValueError, match="non-finite"):
        cnv.tl.tsne(None, use_rep=x, init_pos=torch.full((300, 2), float("inf")).cuda(), **kw)
    with pytest.raises(ValueError, match="init_pos has shape"):
        cnv.tl.tsne(None, use_rep=x, init_pos=np.zeros((300, 3), dtype=np.float32), **kw)

    g = lo.wide_weights()
    bad = g.tolil()
    bad[0, 0] = 1.0
    n = g.shape[0]

    def run(m_or_dev):
        dev = m_or_dev if isinstance(m_or_dev, tuple) else _device(m_or_dev)
        y = torch.from_numpy(to.random_init(n, 2, 0)).cuda()
        before = y.clone()
        try:
            _engine.tsne_iterations(*dev, y, torch.zeros_like(y), torch.ones_like(y), iter_begin=0, iter_end=2)
        finally:
            assert torch.equal(y, before)  # nothing is touched before the validation has passed

    for m, what in ((bad.tocsr(), "diagonal"), (sp.triu(g).tocsr(), "symmetric"), (-g, "negative"), (g * np.inf, "finite"),
                    (g * 4.0, "above 2")):
        with pytest.raises(ValueError, match=what):
            run(m)
    indptr, indices, data = _device(g)
    for wrong in (indptr + 1, indptr * 2, torch.flip(indptr, (0,))):
        with pytest.raises(ValueError, match="indptr"):
            run((wrong, indices, data))


def test_chain_up_to_pl_tsne_on_golden():
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
    n = g.X.shape[0]
    cnv.tl.tsne(ad, perplexity=min(30, (n - 1) // 4))
    cnv.tl.leiden(ad)
    assert ad.obsm["X_cnv_tsne"].shape == (n, 2) and np.isfinite(ad.obsm["X_cnv_tsne"]).all()
    ax = cnv.pl.tsne(ad, color="cnv_leiden")
    try:
        assert len(ax.collections[0].get_offsets()) == n
        assert ax.get_legend() is not None
        assert ax.get_xlabel() == "cnv_tsne1" and ax.get_ylabel() == "cnv_tsne2"
    finally:
        plt.close(ax.figure)

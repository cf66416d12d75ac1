"""tl.leiden without a GPU: the numpy oracle against the guarantees of the Leiden paper and against
networkx's Louvain, exact answers that follow from the contract, and the argument validation of cnv.tl.leiden."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import _leiden_oracle as lo  # noqa: E402
import make_leiden_golden as mg  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "leiden", "louvain_q.npz")
GAMMAS = (0.5, 1.0, 2.0)
LEIDEN_SYMBOLS = ("icv_leiden_workspace", "icv_leiden_quantise", "icv_leiden_iteration", "icv_leiden_sums",
                  "icv_leiden_renumber")
_cache = {}


def _graph(name):
    if name not in _cache:
        _cache[name] = lo.mixture_graph(int(name[3:]), 0) if name.startswith("mix") else lo.small_graphs()[name]
    return _cache[name]


NAMES = tuple(lo.small_graphs()) + ("mix2000",)


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("name", NAMES)
def test_partition_connected_and_node_optimal(name, gamma):
    g = _graph(name)
    labels, info = lo.leiden(g, gamma, 0, -1, True, return_info=True)
    assert labels.shape == (g.shape[0],) and labels.dtype == np.int32
    lo.check_partition(labels)
    gi = lo.int_graph(g)
    lo.check_connected(gi, labels)
    assert not info["bound_reached"], info
    lo.check_node_optimal(gi, labels, gamma)


@pytest.mark.parametrize("n", (2000, 5000))
def test_quality_against_louvain(n):
    gold = np.load(GOLDEN)
    g = _graph(f"mix{n}")
    try:
        import networkx  # noqa: F401

        G = mg.nx_graph(g)
    except ImportError:
        G = None
    for gamma in GAMMAS:
        q = gold[mg.key(n, gamma)]
        assert q.shape == (10,)
        labels = lo.leiden(g, gamma)
        ours = lo.modularity(g, labels, gamma)
        if G is not None:  # "that same networkx function"
            assert abs(mg.labels_q(G, labels, gamma) - ours) < 1e-12
            ours = mg.labels_q(G, labels, gamma)
        print(f"n={n} gamma={gamma}: oracle Q={ours:.6f} Louvain Q in [{q.min():.6f}, {q.max():.6f}]")
        assert ours >= q.min() - (q.max() - q.min()), (n, gamma, ours, q.min(), q.max())
    if G is not None:  # the golden is what networkx gives
        assert abs(mg.louvain_q(G, 1.0, 0) - gold[mg.key(n, 1.0)][0]) < 1e-9


def test_exact_answers():
    sizes = [7, 5, 5, 9, 3, 2, 1]
    labels = lo.leiden(lo.cliques(sizes), 1.0)
    member = np.repeat(np.arange(len(sizes)), sizes)
    assert len(set(zip(member.tolist(), labels.tolist()))) == len(sizes) == labels.max() + 1
    assert np.array_equal(lo.leiden(lo.isolated(17)), np.arange(17))
    assert np.array_equal(lo.leiden(lo.isolated(1)), [0])
    assert np.array_equal(lo.leiden(lo.path(2), 1.0), [0, 0])
    for name in ("mix2000", "ring_of_cliques", "wide_weights"):  # gamma above 2m max A_ij / min k_i^2: no merge gains
        g = _graph(name)
        gi = lo.int_graph(g)
        k = np.asarray(gi.sum(axis=1)).ravel().astype(np.float64)
        gamma = 1.01 * k.sum() * gi.data.max() / k[k > 0].min() ** 2
        assert np.array_equal(lo.leiden(g, gamma), np.arange(g.shape[0])), name


def test_pure_function_and_random_state():
    g = _graph("mix2000")
    a, ia = lo.leiden(g, 1.0, 0, -1, True, return_info=True)
    b, ib = lo.leiden(g, 1.0, 0, -1, True, return_info=True)
    assert np.array_equal(a, b) and ia == ib
    c = lo.leiden(g, 1.0, 1)
    gi = lo.int_graph(g)
    for lab in (a, c):
        lo.check_partition(lab)
        lo.check_connected(gi, lab)
    u = lo.leiden(g, 1.0, 0, 2, False)
    lo.check_connected(lo.int_graph(g, False), u)
    assert len(ia["quality"]) == ia["n_iterations"] == len(ia["levels"])


def test_quantisation_drops_and_rejects():
    g = lo.wide_weights()
    indptr, indices, w = lo.quantise(g)
    assert indptr[-1] < g.nnz and w.min() >= 1 and w.max() == 1 << 32
    bad = g.tolil()
    bad[0, 0] = 1.0
    for m, what in ((bad.tocsr(), "diagonal"), (sp.triu(g).tocsr(), "symmetric"), (-g, "negative"),
                    (g * np.inf, "finite"), (g * 2.0 ** 40, "too large"), (sp.csr_matrix((3, 4)), "square")):
        with pytest.raises(ValueError, match=what):
            lo.quantise(m)


def test_argument_validation_touches_no_gpu():
    import infercnvpy_amd as cnv
    from infercnvpy_amd._compat import SimpleAnnData

    g = lo.path(6)
    ad = SimpleAnnData(np.zeros((6, 3), dtype=np.float32))
    for kw in ("restrict_to", "partition_type", "flavor", "foo"):
        with pytest.raises(ValueError, match=kw):
            cnv.tl.leiden(ad, adjacency=g, **{kw: 1})
    for kw in ({"resolution": -1.0}, {"resolution": float("nan")}, {"resolution": "x"}, {"n_iterations": 0},
               {"n_iterations": 1.5}, {"n_iterations": -2}, {"random_state": 0.5}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cnv.tl.leiden(ad, adjacency=g, **kw)
    with pytest.raises(KeyError, match="pp.neighbors"):
        cnv.tl.leiden(ad)
    with pytest.raises(KeyError, match="pp.neighbors"):
        cnv.tl.leiden(ad, obsp="nope")
    ad.uns["cnv_neighbors"] = {"connectivities_key": "gone"}
    with pytest.raises(KeyError, match="pp.neighbors"):
        cnv.tl.leiden(ad)
    with pytest.raises(ValueError, match="square"):
        cnv.tl.leiden(ad, adjacency=sp.csr_matrix((6, 5)))
    with pytest.raises(ValueError, match="6 cells"):
        cnv.tl.leiden(ad, adjacency=lo.path(5))
    with pytest.raises(ValueError, match="scipy sparse"):
        cnv.tl.leiden(ad, adjacency=np.zeros((6, 6)))


def test_leiden_symbols_are_exported_and_declared():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                               "infercnv_hip.h")).read()
    for name in LEIDEN_SYMBOLS:
        assert name in _lib.EXPORTS
        assert getattr(lib, name) is not None
        assert f"int {name}(" in header, name


def test_workspace_is_linear_and_validates():
    import ctypes as C

    from infercnvpy_amd import _lib

    lib = _lib.load()
    b = [C.c_int64(0) for _ in range(3)]
    for out, (n, nnz) in zip(b, ((1000, 28000), (2000, 56000), (4000, 112000))):
        assert lib.icv_leiden_workspace(n, nnz, C.byref(out)) == 0
    assert b[0].value < b[1].value < b[2].value
    assert abs((b[2].value - b[1].value) - 2 * (b[1].value - b[0].value)) < 64 * 1024
    assert b[2].value <= 128 * 4000 + 80 * 112000 + (1 << 16)
    assert lib.icv_leiden_workspace(0, 0, C.byref(b[0])) == _lib.ICV_ERR_INVALID

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


# ---- the edge builders of test_gpu_leiden_edges.py: the oracle itself reaches the branch each of them is for ----------
def _stats_run(g, gamma=1.0, rs=0, nit=1):
    st = lo.new_stats()
    labels, info = lo.leiden(g, gamma, rs, nit, True, return_info=True, stats=st)
    return labels, info, st


def _lengths(st, level):
    return set().union(*(set(u.tolist()) for lv, u in st["row_lengths"] if lv == level))


def test_iteration_is_the_body_of_leiden_and_stats_only_observe():
    g = _graph("wide_weights")
    indptr, indices, w = lo.quantise(g)
    gom = 1.0 / float(sum(int(x) for x in w))
    labels, info = lo.leiden(g, 1.0, 5, -1, True, return_info=True)
    cur = np.arange(g.shape[0])
    for it in range(info["n_iterations"]):
        plain = lo.iteration(indptr, indices, w, gom, 5, it, cur)
        st = lo.new_stats()
        counted = lo.iteration(indptr, indices, w, gom, 5, it, cur, st)
        assert np.array_equal(plain[0], counted[0]) and plain[1:] == counted[1:]
        assert plain[1] == info["levels"][it] and plain[2] == info["rounds"][it] and not plain[4]
        assert (st["thinned"] > 0) == (plain[3] > 0) and st["blocked"] > 0 and len(st["row_lengths"]) == len(plain[1])
        cur = plain[0]
    assert plain[3] == 0 and np.array_equal(lo.renumber(cur), labels)
    assert np.array_equal(cur, lo.converged(g, 1.0, 5)[0])


def test_rows_at_split_has_rows_around_512():
    _, info, st = _stats_run(lo.rows_at_split())
    assert {511, 512, 513, 514} <= _lengths(st, 0) and info["levels"] == [[1539, 3]]
    assert st["tie_lower_id"] > 0  # a clique: every neighbouring singleton has the same gain
    # the hub variant has such rows at level 1 as well (gamma = 2: all five hubs stay alone on the aggregate)
    g = lo.pairs_with_hubs()
    assert g.shape[0] == 1035
    _, info, st = _stats_run(g, 2.0)
    assert {511, 512, 513, 514, 515} <= _lengths(st, 0) and {511, 512, 513, 514, 515} <= _lengths(st, 1)
    assert info["levels"][0][:2] == [1035, 520]
    _, _, st = _stats_run(g, 1.0)
    assert max(_lengths(st, 1)) == 514


def test_heavy_mixed_rounds_its_conversions():
    g = lo.heavy_mixed()
    indptr, indices, w = lo.quantise(g)
    total = sum(int(x) for x in w)
    assert len(w) == 1170 and 0.14 * 2 ** 62 < total < 0.15 * 2 ** 62
    labels, _, st = _stats_run(g, 1.0, 0, -1)
    assert st["inexact_gain"] > 0 and st["inexact_wellconn"] > 0
    _, K = lo.community_sums(indptr, indices, w, labels)
    inexact = [int(float(int(k))) != int(k) for k in K]
    assert len(K) == 34 and sum(inexact) >= 10 and all(inexact[:4])  # the largest K_c are not float64 numbers


def test_near_limit_sums():
    graphs = lo.near_limit()
    _, _, w = lo.quantise(graphs["pair_below"])
    assert sum(int(x) for x in w) == 2 ** 62 - 2 ** 38
    _, _, w = lo.quantise(graphs["mixed_below"])
    assert 0.875 * 2 ** 62 < sum(int(x) for x in w) < 2 ** 62 and {3, 5} <= set(w.tolist())
    _, _, st = _stats_run(graphs["mixed_below"])
    assert st["inexact_gain"] > 0 and st["inexact_wellconn"] > 0
    for name in ("over_pair", "over_k3"):
        assert graphs[name].data.max() < 2.0 ** 30  # not the per-value limit: the sum decides
        with pytest.raises(ValueError, match="too large"):
            lo.quantise(graphs[name])
    _, _, w = lo.quantise(graphs["over_pair"] * (1 - 2.0 ** -24))
    assert sum(int(x) for x in w) == 2 ** 62 - 2 ** 38


def test_rint_ties_round_to_even():
    g = lo.rint_ties()
    assert g.nnz == 22 and np.array_equal(g.data.astype(np.float32).astype(np.float64), g.data)
    assert 0 < g.data.min() < 2.0 ** -126  # the subnormal
    indptr, indices, w = lo.quantise(g)
    got = sp.csr_matrix((w, indices, indptr), shape=g.shape)
    n = g.shape[0]
    assert [int(got[i, i + 1]) for i in range(9)] == [0, 1, 2, 2, 2, 3, 4, 4, 4]  # (i + 1) / 2, ties to even
    assert got[9, 10] == 0 and got[10, 0] == 1 << 32 and got.nnz == 18 and (got != got.T).nnz == 0 and n == 11


@pytest.mark.parametrize("name", tuple(lo.EMPTIES_CASES))
def test_empties_run_out_of_free_ids(name):
    n, members, seed = lo.EMPTIES_CASES[name]
    assert lo.empties_search(n, members) == seed  # the committed seed is the first of the fixed range [0, 4096)
    g, labels = lo.empties_run_out(n, members)
    assert np.bincount(labels, minlength=n).max() == members and (np.bincount(labels, minlength=n) == 0).sum() == members - 1
    assert not any(g[i, j] for i in range(0, 2 * members, 2) for j in range(0, 2 * members, 2))
    indptr, indices, w = lo.quantise(g)
    gom = lo.EMPTIES_GAMMA / float(sum(int(x) for x in w))
    for it in lo.EMPTIES_ITS:
        st = lo.new_stats()
        out, levels, rounds, moves, bound = lo.iteration(indptr, indices, w, gom, seed, it, labels, st)
        assert st["empty_short_rounds"] >= 1 and st["empty_got_none"] >= 1 and not bound, (it, st)
        assert moves == members - 1 and len(set(out.tolist())) == n  # every free id was handed out: all singletons


def test_zero_gain_refinement_merges():
    for name, (g, gamma) in lo.zero_gain_cases().items():
        indptr, indices, w = lo.quantise(g)
        st = lo.new_stats()
        out, levels, rounds, moves, bound = lo.iteration(indptr, indices, w, gamma / float(sum(int(x) for x in w)), 0, 0,
                                                         np.zeros(g.shape[0], dtype=np.int32), st)
        assert st["zero_gain_refine"] > 0 and levels == [g.shape[0], 1] and moves == 0 and not bound, name


def test_kv_not_float32_decides_by_the_low_bit_of_k():
    g, gamma = lo.kv_not_float32()
    indptr, indices, w = lo.quantise(g)
    k = np.array([int(w[indptr[1]:indptr[2]].sum())])
    assert k[0] == 2 ** 32 + 1 and int(np.float32(k[0])) == 2 ** 32
    gom = gamma / float(sum(int(x) for x in w))
    dk = np.array([1 << 32])
    assert lo._gain(gom, dk, k, dk)[0] == -0.25 and lo._gain(gom, dk, np.array([1 << 32]), dk)[0] == 0.75
    labels, info = lo.leiden(g, gamma, 0, -1, True, return_info=True)
    assert np.array_equal(labels, [0, 1, 2]) and info["rounds"] == [[(0, 0)]]


@pytest.mark.parametrize("name", ("ring_of_cliques", "wide_weights", "heavy_mixed"))
def test_start_partitions_reach_their_branches(name):
    from scipy.sparse.csgraph import connected_components

    g = lo.heavy_mixed() if name == "heavy_mixed" else _graph(name)
    n = g.shape[0]
    indptr, indices, w = lo.quantise(g)
    gom = 1.0 / float(sum(int(x) for x in w))
    parts = lo.start_partitions(g)
    assert (parts["one"] == 0).all()
    used = np.unique(parts["gaps"])
    assert len(used) <= n // 9 and used.max() - used.min() > n // 2 and not np.array_equal(used, np.arange(len(used)))
    d = parts["disconnected"]
    a = sp.coo_matrix(g)
    keep = d[a.row] == d[a.col]
    inside = sp.csr_matrix((np.ones(keep.sum()), (a.row[keep], a.col[keep])), shape=g.shape)
    assert connected_components(inside, directed=False)[0] > len(np.unique(d))
    parts["converged"], _ = lo.converged(g, 1.0, 0)
    total = lo.new_stats()
    for pname, labels in parts.items():
        assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() < n
        for it in (0, 1, 63):
            st = lo.new_stats()
            out, levels, rounds, moves, bound = lo.iteration(indptr, indices, w, gom, 0, it, labels, st)
            assert not bound and levels[0] == n
            assert (moves == 0) == (pname == "converged"), (pname, it, moves)
            for key in st:
                if key != "row_lengths":
                    total[key] += st[key]
    assert total["empty_rounds"] > 0 and total["refine_candidates_rejected"] > 0 and total["blocked"] > 0
    assert total["empty_got_none"] == 0  # only the empties_run_out cases get there
    if name == "ring_of_cliques":
        assert total["tie_lower_id"] > 0
    if name == "heavy_mixed":
        assert total["refine_movers_rejected"] > 0 and total["inexact_gain"] > 0 and total["inexact_wellconn"] > 0


def test_rule5_bounds():
    """The iteration bound is reached by asking for more; the round bound by no case of the seeded search (DESIGN.md
    4.10 has the full budget's outcome; this is its first slice); the level bound needs 64 levels that each merge."""
    labels, info = lo.leiden(_graph("ring_of_cliques"), 1.0, 0, 100, True, return_info=True)
    assert info["n_iterations"] == lo.MAX_ITERATIONS == 64 and not info["bound_reached"]
    assert np.array_equal(labels, lo.leiden(_graph("ring_of_cliques"), 1.0, 0, -1))
    assert max(g.shape[0] for g in lo.rule5_shapes().values()) == 12
    found, closest = lo.rule5_search(300)
    assert found == [] and closest < 0

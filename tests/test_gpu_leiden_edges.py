"""GPU tests (``-m gpu``): tl.leiden at its row, weight, empty-community and bound limits, against the numpy oracle of
DESIGN.md 4.10 (tests/_leiden_oracle.py).  The inputs are the builders of the oracle file; that the oracle itself
enters the branch each of them is for is asserted on the CPU in tests/test_leiden_oracle.py.  Every comparison is
``np.array_equal`` or ``==``.

What test_gpu_leiden.py does not enter: rows of 511 to 515 entries (the split between k_ld_decide and k_ld_decide_long,
at level 0 and on an aggregate), int64 sums that are not float64 numbers, a sum of weights at 2^62, the ties of rint,
rule 4d running out of free ids, a refinement at gain 0, one iteration from a partition that is neither singletons nor
a previous result, iteration indices above 2, seeds outside [0, 2^63), resolution 0 and 1e9, and the iteration bound."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import _leiden_oracle as lo

pytestmark = pytest.mark.gpu
GAMMAS = (0.5, 1.0, 2.0)
INFO_KEYS = ("levels", "rounds", "n_iterations", "bound_reached", "quality")


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name in ("pair_below", "mixed_below", "over_pair", "over_k3"):
        return lo.near_limit()[name]
    if name == "with_isolated":  # an isolated vertex in the middle of a structured graph
        return sp.block_diag([lo.cliques([5] * 6, ring=True), lo.isolated(1), lo.cliques([4] * 5, ring=True)]).tocsr()
    if name.startswith("empties_"):
        return lo.empties_run_out(*lo.EMPTIES_CASES[name[8:]][:2])[0]
    if name.startswith("zero_"):
        return lo.zero_gain_cases()[name[5:]][0]
    if name in lo.small_graphs():
        return lo.small_graphs()[name]
    return getattr(lo, name)()


def _run(g, **kw):
    import infercnvpy_amd as cnv

    cat, info = cnv.tl.leiden(None, adjacency=g, inplace=False, return_info=True, **kw)
    assert list(cat.categories) == [str(i) for i in range(info["n_communities"])]
    return np.asarray(cat.codes, dtype=np.int32), info


def _same_as_oracle(g, gamma, rs, nit, what):
    got, info = _run(g, resolution=gamma, random_state=rs, n_iterations=nit)
    ref, rinfo = lo.leiden(g, gamma, rs, nit, True, return_info=True)
    assert np.array_equal(got, ref), what
    for key in INFO_KEYS:
        assert info[key] == rinfo[key], (what, key)
    return got, info


def _device_csr(g, dtype=None):
    import torch

    from infercnvpy_amd.tl._leiden import _host_csr

    indptr, indices, data = _host_csr(g)
    return (torch.from_numpy(indptr).cuda(), torch.from_numpy(indices).cuda(),
            torch.from_numpy(data if dtype is None else data.astype(dtype)).cuda())


def _quantise(g, use_weights=True, dtype=None):
    """_engine.leiden_quantise on the host: (indptr, indices, weights, total)."""
    from infercnvpy_amd import _engine

    q_indptr, q_indices, q_w, total = _engine.leiden_quantise(*_device_csr(g, dtype), use_weights)
    return q_indptr.cpu().numpy(), q_indices.cpu().numpy(), q_w.cpu().numpy(), total


@functools.lru_cache(maxsize=None)
def _integer_graph(name):
    """The device's integer graph of _graph(name), its workspace, and the oracle's integer graph (shared, read only)."""
    from infercnvpy_amd import _engine

    g = _graph(name)
    q = _engine.leiden_quantise(*_device_csr(g))
    ref = lo.quantise(g)
    assert q[3] == sum(int(x) for x in ref[2])
    return q, _engine.leiden_workspace(g.shape[0], q[1].numel()), ref


def _iteration_equals_oracle(name, gamma, seed, it, labels, what):
    """One iteration from `labels` on the device and in the oracle; returns the oracle's result."""
    import torch

    from infercnvpy_amd import _engine

    (q_indptr, q_indices, q_w, total), ws, (indptr, indices, w) = _integer_graph(name)
    gom = float(gamma) / float(total)
    dev = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    levels, rounds, moves, bound = _engine.leiden_iteration(q_indptr, q_indices, q_w, gom, seed, it, dev, ws)
    ref = lo.iteration(indptr, indices, w, gom, seed, it, labels)
    assert np.array_equal(dev.cpu().numpy(), ref[0]), what
    assert (levels, rounds, moves, bound) == ref[1:], (what, (levels, rounds, moves, bound), ref[1:])
    return ref


# ---- whole runs --------------------------------------------------------------------------------------------------------
# the oracle needs about 2 s for one run of the 1 539-vertex clique graph: four of the twelve combinations, one per case
@pytest.mark.parametrize("gamma,rs,nit", ((0.5, 0, 1), (1.0, 1, -1), (2.0, 0, -1), (2.0, 1, 1)))
def test_rows_at_the_split_equal_the_oracle(gamma, rs, nit):
    """Rows of 511 / 512 (k_ld_decide) and 513 / 514 entries (k_ld_decide_long) in one graph."""
    _same_as_oracle(_graph("rows_at_split"), gamma, rs, nit, (gamma, rs, nit))


@pytest.mark.parametrize("name", ("pairs_with_hubs", "heavy_mixed", "pair_below", "mixed_below"))
def test_whole_runs_equal_the_oracle(name):
    """pairs_with_hubs: rows of 511 .. 515 entries at level 0 and (gamma = 2) at level 1; heavy_mixed / mixed_below: sums
    beyond 2^53, whose conversions round; pair_below: sum w = 2^62 - 2^38."""
    g = _graph(name)
    for gamma in GAMMAS:
        for rs in (0, 1):
            for nit in (1, -1):
                _, info = _same_as_oracle(g, gamma, rs, nit, (name, gamma, rs, nit))
    if name == "pairs_with_hubs":
        assert info["levels"][0][:2] == [1035, 520]  # gamma = 2: the five hubs are vertices of the aggregate


def test_strength_is_converted_from_int64_directly():
    """k_1 = 2^32 + 1 is no float32 number; through float32 the gain of the only candidate move turns from -0.25 to
    +0.75 (test_leiden_oracle.py::test_kv_not_float32_decides_by_the_low_bit_of_k)."""
    g, gamma = lo.kv_not_float32()
    for rs in (0, 1):
        for nit in (1, -1):
            got, info = _same_as_oracle(g, gamma, rs, nit, (rs, nit))
            assert np.array_equal(got, [0, 1, 2]) and info["rounds"] == [[(0, 0)]]


# ---- one iteration from any partition --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ring_of_cliques", "wide_weights", "heavy_mixed"))
def test_one_iteration_from_any_partition(name):
    g = _graph(name)
    parts = lo.start_partitions(g)
    parts["converged"], _ = lo.converged(g, 1.0, 0)
    for pname, labels in parts.items():
        for it in (0, 1, 63):
            ref = _iteration_equals_oracle(name, 1.0, 0, it, labels, (name, pname, it))
            assert (ref[3] == 0) == (pname == "converged")
    for gamma, seed in ((0.5, 2 ** 64 - 1), (2.0, 2 ** 63 + 11)):
        _iteration_equals_oracle(name, gamma, seed, 17, parts["gaps"], (name, gamma, seed))


@pytest.mark.parametrize("case", tuple(lo.EMPTIES_CASES))
def test_empties_run_out_of_free_ids(case):
    """Rule 4d: more selected vertices want an empty community than ids are free; the last of them (by index) stays."""
    n, members, seed = lo.EMPTIES_CASES[case]
    _, labels = lo.empties_run_out(n, members)
    for it in lo.EMPTIES_ITS:
        ref = _iteration_equals_oracle(f"empties_{case}", lo.EMPTIES_GAMMA, seed, it, labels, (case, it))
        assert ref[3] == members - 1 and len(set(ref[0].tolist())) == n


def test_refinement_merges_at_gain_zero():
    for name, (g, gamma) in lo.zero_gain_cases().items():
        ref = _iteration_equals_oracle(f"zero_{name}", gamma, 0, 0, np.zeros(g.shape[0], dtype=np.int32), name)
        assert ref[1] == [g.shape[0], 1]


# ---- rule 2 alone --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("rint_ties", "wide_weights", "heavy_mixed"))
def test_quantise_equals_the_oracle(name):
    g = _graph(name)
    for dtype in (np.float32, np.float64):
        # float64 values that are no float32 numbers and round back to g (the subnormal of rint_ties included)
        a = g.astype(np.float32) if dtype == np.float32 else g.astype(np.float64) * (1 + 2.0 ** -30)
        assert a.dtype == dtype
        for use_weights in (True, False):
            indptr, indices, w = lo.quantise(a, use_weights)
            q_indptr, q_indices, q_w, total = _quantise(a, use_weights)
            what = (name, dtype.__name__, use_weights)
            assert q_indptr.dtype == np.int64 and q_indices.dtype == np.int32 and q_w.dtype == np.int64
            assert np.array_equal(q_indptr, indptr) and np.array_equal(q_indices, indices), what
            assert np.array_equal(q_w, w), what
            assert len(q_w) == len(w) == indptr[-1] and total == sum(int(x) for x in w), what  # kept, total
            if use_weights and name != "heavy_mixed":
                assert len(w) < g.nnz  # entries were dropped
            if not use_weights:
                assert len(w) == g.nnz and (w == 1 << 32).all()


def test_sum_limit_is_a_value_error():
    """Every value is below 2^30 (flag 64 stays clear): the total of the two 32-bit halves decides."""
    for name in ("over_pair", "over_k3"):
        g = _graph(name)
        assert g.data.max() < 2.0 ** 30
        for dtype in (np.float32, np.float64):
            with pytest.raises(ValueError, match="too large"):
                _quantise(g, True, dtype)
        with pytest.raises(ValueError, match="too large"):
            _run(g)
        _, _, w, total = _quantise(g, False)  # without the weights the same graph is accepted
        assert total == g.nnz << 32 and (w == 1 << 32).all()
    below = _graph("over_pair") * (1 - 2.0 ** -24)  # one float32 ulp less: accepted
    assert _quantise(below)[3] == 2 ** 62 - 2 ** 38


# ---- arguments at their limits ---------------------------------------------------------------------------------------------
def test_random_state_outside_int63():
    g = _graph("ring_of_cliques")
    for rs in (-1, 2 ** 63 + 5, 2 ** 64 - 1, 2 ** 64 + 3):
        got, _ = _same_as_oracle(g, 1.0, rs, -1, rs)
    three, _ = _run(g, random_state=3)
    assert np.array_equal(got, three)  # the seed is taken modulo 2^64


def test_resolution_zero_and_huge():
    from scipy.sparse.csgraph import connected_components

    g = _graph("cliques")
    got, info = _same_as_oracle(g, 0.0, 0, -1, "gamma 0")
    ncomp, comp = connected_components(g, directed=False)
    assert info["n_communities"] == ncomp == 7 and len(set(zip(comp.tolist(), got.tolist()))) == ncomp
    for name in ("cliques", "ring_of_cliques", "with_isolated"):
        got, _ = _same_as_oracle(_graph(name), 0.0, 1, 2, (name, "gamma 0"))
    g = _graph("ring_of_cliques")
    got, info = _same_as_oracle(g, 1e9, 0, -1, "gamma 1e9")
    assert np.array_equal(got, np.arange(g.shape[0])) and info["n_iterations"] == 1
    assert info["levels"] == [[g.shape[0]]] and info["rounds"] == [[(0, 0)]]
    ref = _iteration_equals_oracle("ring_of_cliques", 1e9, 0, 0, np.arange(g.shape[0], dtype=np.int32), "gamma 1e9")
    assert ref[3] == 0 and np.array_equal(ref[0], np.arange(g.shape[0]))


def test_isolated_vertex_inside_a_structured_graph():
    g = _graph("with_isolated")
    assert g.shape[0] == 51 and g.indptr[31] == g.indptr[30]
    for gamma in GAMMAS:
        for nit in (1, -1):
            got, _ = _same_as_oracle(g, gamma, 0, nit, (gamma, nit))
            assert (got == got[30]).sum() == 1  # alone


def test_iteration_bound():
    """n_iterations above the bound of rule 5 runs 64 iterations; that is not `bound_reached`."""
    got, info = _same_as_oracle(_graph("ring_of_cliques"), 1.0, 0, 100, "n_iterations=100")
    assert info["n_iterations"] == 64 and not info["bound_reached"] and len(info["levels"]) == 64

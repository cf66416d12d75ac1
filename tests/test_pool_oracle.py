"""The oracle of tl.cnv_pool_neighbors (tests/_pool_oracle.py) against an independent exact mean, what the
planted case of DESIGN.md 4.18 gains from pooling, and everything tl.cnv_pool_neighbors and its two entry points refuse
before they touch the device.  No GPU."""
import ctypes
import fractions
import functools
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _correlation_oracle as co
import _pool_oracle as po
import _pseudobulk_oracle as pb
import _states_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTED_CHR_POS = {"chr1": 0, "chr2": 90, "chr3": 180}


# ---- the oracle against an independent exact mean ------------------------------------------------------------------------------
def test_oracle_equals_an_exact_fraction_mean_on_a_non_symmetric_graph():
    x = pb.random_sparse(23, 31, 0.4, 3)
    graph = po.random_graph(23, 6, 4, diagonal_row=2)
    assert (graph != graph.T).nnz > 0
    got = po.pool(x, graph)
    dense = x.toarray()
    hoods = po.neighbourhoods(graph, 23)
    assert hoods[0].tolist() == [0] and hoods[2].tolist().count(2) == 1 and len(hoods[2]) == 3
    assert got["n_cells"].dtype == np.int32 and got["n_cells"].tolist() == [len(h) for h in hoods]
    assert got["largest"] == 7 and got["shift"] == 40
    for i, hood in enumerate(hoods):
        for j in range(31):
            # (round() of a Fraction is exact and ties to even: rule 4 without a float)
            total = sum(round(fractions.Fraction(float(dense[r, j])) * 2 ** 40) for r in hood)
            want = pb.exact_mean(total, len(hood), 40)
            assert np.float64(want).tobytes() == got["pooled"][i, j].tobytes(), (i, j)
    assert not np.signbit(got["pooled"][got["pooled"] == 0]).any()  # S = 0 gives +0.0


def test_only_the_structure_of_the_graph_counts():
    x = pb.random_sparse(23, 31, 0.4, 3)
    graph = po.random_graph(23, 6, 4)
    other = graph.copy()
    other.data[:] = 0.0  # explicit zeros are entries
    as_tuple = (graph.indptr, graph.indices)
    want = po.pool(x, graph)["pooled"].tobytes()
    assert po.pool(x, other)["pooled"].tobytes() == want and po.pool(x, as_tuple)["pooled"].tobytes() == want
    assert po.pool(x.toarray(), graph)["pooled"].tobytes() == want
    assert po.pool(x, po.edgeless(23))["n_cells"].tolist() == [1] * 23


def test_the_case_builders_hold_what_the_gpu_tests_rely_on():
    c = po.storage_case()
    lens = np.diff(c["graph"].indptr)
    assert c["x"].shape == (37, 70) and lens.min() == 0 and lens.max() in (9, 10)
    assert (c["x"].data == 0).any() and np.signbit(c["x"].data[c["x"].data == 0]).any()
    for w in (po.TILE - 1, po.TILE, po.TILE + 1, 2 * po.TILE + 3):
        d = po.tile_edges_case(w)["x"].toarray()
        assert d.shape == (9, w) and (d[:, w - 1] != 0).any()
        for t in range(po.TILE, w + 1, po.TILE):
            assert (d[:, t - 1] != 0).any() and (t >= w or (d[:, t] != 0).any())
    c = po.graph_rows_case()
    lens = np.diff(c["graph"].indptr)
    assert lens[:7].tolist() == [700, 0, 1, 63, 64, 65, 1] and lens[0] > po.GRAPH_LONG_ROW
    assert po.pool(c["x"], c["graph"])["n_cells"][:7].tolist() == [701, 1, 2, 64, 65, 66, 1]
    c = po.matrix_rows_case()
    got = po.pool(c["x"], c["graph"])
    assert (got["pooled"][:3].view(np.int64) == 0).all() and (got["pooled"][3:] != 0).any()
    c = po.hub_case()
    got = po.pool(c["x"], c["graph"])
    assert got["largest"] == 4097 and got["shift"] == 39
    c = pb.big_sum_case()
    got = po.pool(c["x"], po.complete(64))
    assert got["shift"] == 40 and got["S"][0].tolist() == c["want_S"]
    floats = c["x"].sum(axis=0) / 64.0  # a floating-point sum of the same rows
    assert (floats.view(np.int64) != got["pooled"][0].view(np.int64)).any()
    c = pb.ties_case()
    got = po.pool(c["x"], po.edgeless(1))
    assert got["shift"] == 40 and (got["pooled"][0] == c["want_q"].astype(np.float64) * 2.0 ** -40).all()


# ---- the planted claim of the issue: what pooling buys -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted_counts(seed):
    c = co.planted(seed)
    graph = po.planted_graph(c["x"], 15)
    assert (np.diff(graph.indptr) == 14).all()
    same = c["clone"][graph.indices].reshape(240, 14) == c["clone"][:, None]
    pooled = po.pool(c["x"], graph)
    raw_states, _, _ = so.cnv_states(c["x"], PLANTED_CHR_POS)
    pooled_states, _, _ = so.cnv_states(pooled["pooled"], PLANTED_CHR_POS)
    tumour = c["clone"] >= 0
    residual = (pooled["pooled"][tumour] - c["truth"][c["clone"][tumour]]).std()
    return (po.wrong_calls(raw_states, c["clone"], c["truth"]), po.wrong_calls(pooled_states, c["clone"], c["truth"]),
            float(same.mean()), float(residual))


@pytest.mark.parametrize("seed", [0, 1])
def test_pooling_the_planted_case_turns_most_wrong_calls_right(seed):
    raw, pooled, same, residual = planted_counts(seed)
    print(f"seed {seed}: {raw} of 64800 raw calls wrong, {pooled} pooled; {same:.3f} of the neighbours in the cell's own "
          f"clone; residual sd {residual:.4f}")
    assert raw >= 14000
    assert pooled <= 500


# ---- what tl.cnv_pool_neighbors refuses before it touches the device -----------------------------------------------------------
def _adata(n=6, w=10, x=None, chr_pos=None, graph="default"):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32), obs=pd.DataFrame({"clone": list("aabbcc")[:n]}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    if graph is not None:
        ad.obsp["cnv_neighbors_distances"] = po.edgeless(n) if isinstance(graph, str) else graph
        ad.uns["cnv_neighbors"] = {"connectivities_key": "cnv_neighbors_connectivities",
                                   "distances_key": "cnv_neighbors_distances"}
    return ad


def _no_chr_pos():
    ad = _adata()
    del ad.uns["cnv"]["chr_pos"]
    return ad


def _no_distances():
    ad = _adata()
    del ad.obsp["cnv_neighbors_distances"]
    return ad


W = "tl.cnv_pool_neighbors: "
BAD = [
    ("missing obsm key", _adata, {"use_rep": "other"}, KeyError, W + "X_other not found in adata.obsm. Did you run `tl.infercnv`?"),
    ("missing chr_pos", _no_chr_pos, {}, KeyError, W + "chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
    ("1-D X", lambda: _adata(x=np.ones(6)), {}, ValueError, W + "X_cnv must be 2-D"),
    ("empty shape", lambda: _adata(x=np.ones((6, 0))), {}, ValueError, W + "empty matrix of shape (6, 0)"),
    ("chr_pos outside", lambda: _adata(chr_pos={"chr1": 0, "chr2": 10}), {}, ValueError,
     W + "chr_pos start 10 is outside [0, 10)"),
    ("missing neighbors_key", lambda: _adata(graph=None), {}, KeyError,
     "'cnv_neighbors' is not in adata.uns. Did you run `pp.neighbors`?"),
    ("missing obsp key", _adata, {"obsp": "nope"}, KeyError, "'nope' is not in adata.obsp. Did you run `pp.neighbors`?"),
    ("missing distances", _no_distances, {}, KeyError,
     "'cnv_neighbors_distances' is not in adata.obsp. Did you run `pp.neighbors`?"),
    ("graph not square", _adata, {"adjacency": sp.csr_matrix((6, 5))}, ValueError, W + "the adjacency matrix must be square"),
    ("graph of no vertices", _adata, {"adjacency": sp.csr_matrix((0, 0))}, ValueError, W + "the adjacency matrix is empty"),
    ("graph of n + 1 vertices", _adata, {"adjacency": sp.csr_matrix((7, 7))}, ValueError,
     W + "the graph has 7 vertices, adata has 6 cells"),
    ("matrix of other rows", lambda: _adata(x=np.ones((5, 10))), {}, ValueError, W + "the graph has 6 vertices, X_cnv has 5 rows"),
    ("a dense graph", _adata, {"adjacency": np.zeros((6, 6))}, ValueError,
     W + "the graph must be a scipy sparse matrix or (indptr, indices, data) CUDA tensors"),
]


@pytest.mark.parametrize("cid, make, kw, kind, message", BAD, ids=[c[0] for c in BAD])
def test_every_bad_input_has_its_exception_and_its_whole_message(cid, make, kw, kind, message):
    import infercnvpy_amd as cnv

    ad = make()
    with pytest.raises(kind) as info:
        cnv.tl.cnv_pool_neighbors(ad, **kw)
    assert type(info.value) is kind and info.value.args[0] == message
    assert "X_cnv_pooled" not in ad.obsm and "cnv_pooled" not in ad.uns


def test_the_three_earlier_callers_still_take_the_connectivities():
    from infercnvpy_amd.tl import _graph

    ad = _adata()
    ad.obsp["cnv_neighbors_connectivities"] = po.complete(6)
    assert _graph._graph(ad, "cnv_neighbors", None, None) is ad.obsp["cnv_neighbors_connectivities"]
    assert _graph._graph(ad, "cnv_neighbors", None, None, "distances_key") is ad.obsp["cnv_neighbors_distances"]
    assert _graph.graph_source(ad, "cnv_neighbors", None, None, "distances_key") == "cnv_neighbors_distances"
    assert _graph.graph_source(ad, "cnv_neighbors", po.edgeless(6), "x") == "adjacency"
    host, dev, n = _graph.resolve_graph("tl.leiden", ad, "cnv_neighbors", None, None)
    assert dev is None and n == 6 and host[1].shape[0] == 30
    # explicit zeros stay entries of the canonical host form
    g = sp.csr_matrix((np.zeros(2), np.asarray([1, 0], dtype=np.int32), np.asarray([0, 2, 2])), shape=(2, 2))
    indptr, indices, _ = _graph._host_csr(g, "tl.cnv_pool_neighbors")
    assert indptr.tolist() == [0, 2, 2] and indices.tolist() == [0, 1] and indptr.dtype == np.int64 and indices.dtype == np.int32


# ---- the library and the package, as far as they go without a GPU -----------------------------------------------------------
ENTRIES = ("icv_neighbor_pool_sizes", "icv_neighbor_pool")


def test_symbols_are_exported_declared_and_bound():
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine, _lib

    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "infercnv_hip.h")).read()
    declared = set(re.findall(r"\b(icv_[a-z_0-9]+)\s*\(", header))
    binding = open(os.path.join(ROOT, "infercnvpy_amd", "_engine.py")).read()
    for name in ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None and f"lib.{name}(" in binding
    assert callable(_engine.neighbor_pool_sizes) and callable(_engine.neighbor_pool)
    assert "cnv_pool_neighbors" in cnv.tl.__all__ and callable(cnv.tl.cnv_pool_neighbors)
    source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_pool.hpp")).read()
    assert f"kPoolTile = {po.TILE};" in source  # (the size the edge cases are built around)
    graph_source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_graph.hpp")).read()
    assert f"kGraphLongRow = {po.GRAPH_LONG_ROW};" in graph_source


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    sizes = lib.icv_neighbor_pool_sizes
    good = [one, one, 4, one, one, None]
    for position, value in ((0, None), (1, None), (2, 0), (2, -1), (3, None), (4, None)):
        args = list(good)
        args[position] = value
        assert sizes(*args) == bad, (position, value)
    assert b"neighbor_pool_sizes" in lib.icv_last_error()

    pool = lib.icv_neighbor_pool
    for fmt in (_lib.ICV_DENSE, _lib.ICV_CSR):
        m = _lib.Matrix()
        m.format, m.dtype, m.n_rows, m.n_cols, m.ld, m.values, m.indptr, m.indices = fmt, _lib.ICV_F64, 4, 5, 5, 8, 8, 8
        good = [ctypes.byref(m), one, one, 4, 40, one, one, 5, one, None]
        for position, value in ((0, None), (1, None), (2, None), (3, 0), (3, -1), (3, 5), (4, -1), (4, 41), (5, None),
                                (6, None), (7, 4), (8, None)):
            args = list(good)
            args[position] = value
            assert pool(*args) == bad, (fmt, position, value)
        fields = [("n_cols", 0), ("n_rows", 3), ("dtype", 7), ("format", 7)]
        fields += [("ld", 4), ("values", None)] if fmt == _lib.ICV_DENSE else [("indptr", None)]
        for field, value in fields:
            keep = getattr(m, field)
            setattr(m, field, value)
            assert pool(*good) == bad, (fmt, field)
            setattr(m, field, keep)
        assert b"neighbor_pool" in lib.icv_last_error() and b"sizes" not in lib.icv_last_error()

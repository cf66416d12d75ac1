"""tl.cnv_pool_neighbors on the GPU equals the oracle of DESIGN.md 4.21 (tests/_pool_oracle.py) on the float64 bytes: for
every storage of the matrix and of the graph, at the edges of the window tile, for graph rows and matrix rows of every
length the kernel treats differently, at the rounding ties and past what a float64 sum holds, with the shift a hub
lowers; it refuses what the contract excludes, and the per-cell HMM calls the planted clones from the pooled rows."""
import functools

import numpy as np
import pandas as pd
import pytest

import _correlation_oracle as co
import _pool_oracle as po
import _pseudobulk_oracle as pb
import _states_oracle as so

pytestmark = pytest.mark.gpu

PLANTED_CHR_POS = {"chr1": 0, "chr2": 90, "chr3": 180}


def _adata(x, chr_pos=None, n=None):
    from infercnvpy_amd._compat import SimpleAnnData

    n = x.shape[0] if n is None else n
    ad = SimpleAnnData(np.zeros((n, 2), dtype=np.float32), obs=pd.DataFrame({"half": np.where(np.arange(n) % 2, "odd", "even")}))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0} if chr_pos is None else dict(chr_pos)}
    return ad


def _cuda_graph(graph):
    import torch

    g = graph.tocsr()
    return (torch.from_numpy(g.indptr.astype(np.int64)).cuda(), torch.from_numpy(g.indices.astype(np.int32)).cuda(),
            torch.from_numpy(g.data.astype(np.float32)).cuda())


def _pool(x, graph, **kw):
    """(pooled as a host array, n_cells, info) of one call with ``adjacency=graph``."""
    import torch

    import infercnvpy_amd as cnv

    pooled, n_cells, info = cnv.tl.cnv_pool_neighbors(_adata(x), adjacency=graph, inplace=False, return_info=True, **kw)
    if torch.is_tensor(pooled):
        pooled = pooled.cpu().numpy()
    return pooled, n_cells, info


def _same(got, want):
    pooled, n_cells, info = got
    assert isinstance(pooled, np.ndarray) and pooled.dtype == np.float64 and pooled.shape == want["pooled"].shape
    assert n_cells.dtype == np.int32 and np.array_equal(n_cells, want["n_cells"])
    assert info["shift"] == want["shift"] and info["largest"] == want["largest"]
    differ = np.flatnonzero(pooled.view(np.int64).ravel() != want["pooled"].view(np.int64).ravel())
    assert differ.shape[0] == 0, (differ[:5], pooled.ravel()[differ[:5]], want["pooled"].ravel()[differ[:5]])


def _inputs(x):
    import torch

    import infercnvpy_amd as cnv

    dense32 = x.toarray().astype(np.float32)
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), torch.from_numpy(x.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(x.data).cuda(), x.shape[1])
    return {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
            "dense_float64": dense32.astype(np.float64), "cuda_float32": torch.from_numpy(dense32).cuda(),
            "cuda_float64": torch.from_numpy(dense32.astype(np.float64)).cuda(), "packed_csr": packed}


@functools.lru_cache(maxsize=None)
def storage():
    c = po.storage_case()
    want = po.pool(c["x"], c["graph"])
    assert want["shift"] == 40 and (want["pooled"] != 0).any() and (want["n_cells"] == 1).any()
    return c["x"], c["graph"], want


# ---- 1. storage -----------------------------------------------------------------------------------------------------------------
def test_every_storage_of_the_matrix_and_of_the_graph_gives_the_oracles_bytes():
    import torch

    import infercnvpy_amd as cnv

    x, graph, want = storage()
    for gname, g in (("scipy", graph), ("cuda", _cuda_graph(graph))):
        for name, xin in _inputs(x).items():
            ad = _adata(xin)
            info = cnv.tl.cnv_pool_neighbors(ad, adjacency=g, return_info=True)
            pooled, n_cells = ad.obsm["X_cnv_pooled"], np.asarray(ad.obs["cnv_pooled_n_cells"])
            if name.startswith(("cuda", "packed")):
                assert torch.is_tensor(pooled) and pooled.is_cuda and pooled.dtype == torch.float64, (gname, name)
                pooled = pooled.cpu().numpy()
            else:
                assert isinstance(pooled, np.ndarray), (gname, name)
            _same((pooled, n_cells, info), want)
            assert set(info) == {"shift", "largest", "stage_ms"} and set(info["stage_ms"]) == {"upload", "sizes", "pool"}
            assert ad.uns["cnv_pooled"] == {"chr_pos": {"chr1": 0}, "params": {"shift": 40, "largest": want["largest"]},
                                            "use_rep": "cnv", "graph": "adjacency"}
            assert ad.uns["cnv_pooled"]["chr_pos"] is not ad.uns["cnv"]["chr_pos"] and ad.obsm["X_cnv"] is xin


def test_the_graph_is_found_under_its_keys_and_inplace_false_writes_nothing():
    import infercnvpy_amd as cnv

    x, graph, want = storage()
    ad = _adata(x)
    ad.obsp["cnv_neighbors_distances"] = graph
    ad.obsp["cnv_neighbors_connectivities"] = po.edgeless(37)
    ad.obsp["mine"] = po.edgeless(37)
    ad.uns["cnv_neighbors"] = {"connectivities_key": "cnv_neighbors_connectivities", "distances_key": "cnv_neighbors_distances"}
    pooled, n_cells = cnv.tl.cnv_pool_neighbors(ad, inplace=False)
    _same((pooled, n_cells, {"shift": 40, "largest": want["largest"]}), want)
    assert set(ad.obsm) == {"X_cnv"} and set(ad.uns) == {"cnv", "cnv_neighbors"} and list(ad.obs.columns) == ["half"]
    cnv.tl.cnv_pool_neighbors(ad, key_added="a")
    cnv.tl.cnv_pool_neighbors(ad, key_added="b", obsp="mine")
    assert ad.uns["a"]["graph"] == "cnv_neighbors_distances" and ad.uns["b"]["graph"] == "mine"
    assert ad.obsm["X_a"].tobytes() == want["pooled"].tobytes()
    alone = po.pool(x, po.edgeless(37))  # every cell on its own: the values rounded to 2^-40
    assert ad.obsm["X_b"].tobytes() == alone["pooled"].tobytes() and np.asarray(ad.obs["b_n_cells"]).tolist() == [1] * 37


# ---- 2. tile edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [po.TILE - 1, po.TILE, po.TILE + 1, 2 * po.TILE + 3])
def test_tile_edges_csr_and_dense_float32(w):
    c = po.tile_edges_case(w)
    want = po.pool(c["x"], c["graph"])
    assert (want["pooled"][:, w - 1] != 0).any()
    _same(_pool(c["x"], c["graph"]), want)
    _same(_pool(c["x"].toarray().astype(np.float32), c["graph"]), want)
    _same(_pool(c["x"].toarray(), c["graph"]), want)


# ---- 3. graph row lengths ---------------------------------------------------------------------------------------------------------
def test_graph_rows_of_every_length():
    c = po.graph_rows_case()
    want = po.pool(c["x"], c["graph"])
    assert want["n_cells"][:7].tolist() == [701, 1, 2, 64, 65, 66, 1] and want["shift"] == 40
    _same(_pool(c["x"], c["graph"]), want)
    _same(_pool(c["x"].toarray(), _cuda_graph(c["graph"])), want)


# ---- 4. matrix row lengths --------------------------------------------------------------------------------------------------------
def test_matrix_rows_of_every_length_and_a_neighbourhood_of_empty_rows():
    c = po.matrix_rows_case()
    want = po.pool(c["x"], c["graph"])
    for xin in (c["x"], c["x"].toarray().astype(np.float64)):
        got = _pool(xin, c["graph"])
        _same(got, want)
        assert (got[0][:3].view(np.int64) == 0).all()  # +0.0, no -0.0 byte


# ---- 5. rounding ------------------------------------------------------------------------------------------------------------------
def test_ties_round_to_even():
    c = pb.ties_case()
    pooled, n_cells, info = _pool(c["x"], po.edgeless(1))
    assert info["shift"] == 40 and n_cells.tolist() == [1]
    assert pooled.tobytes() == (c["want_q"].astype(np.float64) * 2.0 ** -40).reshape(1, -1).tobytes()


def test_sums_past_the_float64_mantissa_are_exact():
    c = pb.big_sum_case()
    graph = po.complete(64)
    want = po.pool(c["x"], graph)
    assert want["shift"] == 40 and want["S"][0].tolist() == c["want_S"] and min(c["want_S"]) > 2 ** 53
    got = _pool(c["x"], graph)
    _same(got, want)
    floats = c["x"].sum(axis=0) / 64.0  # a float64 accumulation of the same rows gives other bytes
    assert (floats.view(np.int64) != got[0][0].view(np.int64)).any()


# ---- 6. shift ---------------------------------------------------------------------------------------------------------------------
def test_a_hub_lowers_the_shift_of_every_cell():
    c = po.hub_case()
    want = po.pool(c["x"], c["graph"])
    assert want["shift"] == 39 and want["largest"] == 4097
    _same(_pool(c["x"], c["graph"]), want)


# ---- 7. determinism ---------------------------------------------------------------------------------------------------------------
def test_two_calls_agree_and_pooling_twice_is_the_oracle_twice():
    import torch

    import infercnvpy_amd as cnv

    x, graph, want = storage()
    assert _pool(x, graph)[0].tobytes() == _pool(x, graph)[0].tobytes()
    ad = _adata(torch.from_numpy(x.toarray()).cuda())
    cnv.tl.cnv_pool_neighbors(ad, adjacency=graph)
    cnv.tl.cnv_pool_neighbors(ad, use_rep="cnv_pooled", key_added="cnv_pooled2", adjacency=graph)
    second = ad.obsm["X_cnv_pooled2"]
    assert torch.is_tensor(second) and second.is_cuda and second.dtype == torch.float64
    again = po.pool(want["pooled"], graph)
    assert second.cpu().numpy().tobytes() == again["pooled"].tobytes()
    assert ad.uns["cnv_pooled2"]["use_rep"] == "cnv_pooled" and ad.uns["cnv_pooled2"]["chr_pos"] == {"chr1": 0}


# ---- 8. errors on the device ------------------------------------------------------------------------------------------------------
def test_what_the_device_finds_is_refused():
    import torch

    import infercnvpy_amd as cnv

    x, graph, want = storage()
    who = "tl.cnv_pool_neighbors: "
    for value in (np.nan, np.inf, -np.inf):
        bad = x.copy()
        bad.data[7] = value
        for xin in (bad, bad.toarray()):
            with pytest.raises(ValueError) as info:
                _pool(xin, graph)
            assert info.value.args[0] == who + "X_cnv has non-finite values"
    bad = x.copy()
    bad.data[7] = -1024.0
    with pytest.raises(ValueError) as info:
        _pool(bad, graph)
    assert info.value.args[0] == (who + "X_cnv has a stored value of magnitude 1024.0; the exact sums take magnitudes below "
                                  "1024: rescale the matrix or clip the value")
    # a PackedCsr whose unused buffer tail holds 4096.0 while its stored entries do not
    nnz = x.nnz
    data = torch.cat([torch.from_numpy(x.data).cuda(), torch.full((5,), 4096.0, dtype=torch.float64, device="cuda")])
    indices = torch.cat([torch.from_numpy(x.indices.astype(np.int32)).cuda(), torch.zeros(5, dtype=torch.int32, device="cuda")])
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), indices, data, x.shape[1])
    assert packed.nnz() == nnz
    _same(_pool(packed, graph), want)
    # device graphs
    indptr, indices, data = _cuda_graph(graph)
    outside = indices.clone()
    outside[3] = 37
    with pytest.raises(ValueError) as info:
        _pool(x, (indptr, outside, data))
    assert info.value.args[0] == who + "the graph has a column outside [0, 37)"
    row = int(np.flatnonzero(np.diff(graph.indptr) >= 2)[0])
    a = int(graph.indptr[row])
    descending = indices.clone()
    descending[a], descending[a + 1] = indices[a + 1], indices[a]
    with pytest.raises(ValueError) as info:
        _pool(x, (indptr, descending, data))
    assert info.value.args[0] == who + "the columns of every row of the graph must ascend strictly"
    with pytest.raises(ValueError) as info:
        _pool(x, po.edgeless(38))
    assert info.value.args[0] == who + "the graph has 38 vertices, adata has 37 cells"


# ---- 9. the chain on the planted case ---------------------------------------------------------------------------------------------
def test_the_per_cell_hmm_calls_the_planted_clones_from_the_pooled_rows():
    import infercnvpy_amd as cnv

    c = co.planted(0)
    # (a) the stand-in graph: the CPU numbers hold on the GPU
    graph = po.planted_graph(c["x"], 15)
    want = po.pool(c["x"], graph)
    want_states, _, _ = so.cnv_states(want["pooled"], PLANTED_CHR_POS)
    ad = _adata(c["x"], PLANTED_CHR_POS)
    cnv.tl.cnv_pool_neighbors(ad, adjacency=graph)
    assert ad.obsm["X_cnv_pooled"].tobytes() == want["pooled"].tobytes()
    assert ad.uns["cnv_pooled"]["chr_pos"] == ad.uns["cnv"]["chr_pos"]
    states, _ = cnv.tl.cnv_states(ad, use_rep="cnv_pooled", inplace=False)
    assert states.tobytes() == want_states.tobytes()
    wrong = po.wrong_calls(states, c["clone"], c["truth"])
    print(f"stand-in graph: {wrong} of 64800 pooled calls wrong")
    assert wrong <= 500

    # (b) the project's own graph
    ad = _adata(c["x"], PLANTED_CHR_POS)
    cnv.tl.pca(ad)
    cnv.pp.neighbors(ad)
    cnv.tl.cnv_pool_neighbors(ad)
    assert ad.uns["cnv_pooled"]["graph"] == "cnv_neighbors_distances"
    assert (np.asarray(ad.obs["cnv_pooled_n_cells"]) == 15).all()
    raw, _ = cnv.tl.cnv_states(ad, inplace=False)
    pooled, _ = cnv.tl.cnv_states(ad, use_rep="cnv_pooled", inplace=False)
    raw_wrong = po.wrong_calls(raw, c["clone"], c["truth"])
    pooled_wrong = po.wrong_calls(pooled, c["clone"], c["truth"])
    print(f"tl.pca + pp.neighbors: {raw_wrong} of 64800 raw calls wrong, {pooled_wrong} pooled")
    assert raw_wrong >= 14000 and pooled_wrong * 10 <= raw_wrong


def test_the_heatmap_draws_the_pooled_rows():
    matplotlib = pytest.importorskip("matplotlib")
    matplotlib.use("Agg")
    import infercnvpy_amd as cnv

    x, graph, _ = storage()
    ad = _adata(x, {"chr1": 0, "chr2": 30})
    cnv.tl.cnv_pool_neighbors(ad, adjacency=graph)
    cnv.pl.chromosome_heatmap(ad, use_rep="cnv_pooled", groupby="half", show=False)
    matplotlib.pyplot.close("all")

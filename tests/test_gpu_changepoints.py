"""tl.cnv_changepoints on the GPU equals the oracle of DESIGN.md 4.19 (tests/_changepoint_oracle.py) on the bytes of its
levels and starts: every chromosome length at which the lanes are shared out differently, many chromosomes, every minimum
length and penalty, ties, a chromosome at the cap, every kind of input, the table, and the planted case."""
import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _changepoint_oracle as co
import _states_oracle as so

pytestmark = pytest.mark.gpu


def _adata(x, chr_pos):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32),
                       obs=pd.DataFrame(index=[f"cell{i}" for i in range(x.shape[0])]))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def assert_equal(levels, starts, want, what):
    assert levels.dtype == np.float64 and co.same_bytes(levels, want["levels"]), what
    assert starts.dtype == np.uint8 and co.same_bytes(starts, want["starts"]), what


# ---- the bytes of levels and starts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(co.CASES))
def test_levels_and_starts_are_the_oracles_bytes(name):
    import infercnvpy_amd as cnv

    c = co.expected(name)
    want = c["want"]
    levels, starts, info = cnv.tl.cnv_changepoints(_adata(c["x"], c["chr_pos"]), inplace=False, return_info=True,
                                                   **c["kwargs"])
    assert info["sigma"] == want["sigma"] and info["beta"] == want["beta"]  # (the default sigma bit for bit)
    assert_equal(levels, starts, want, name)
    lengths = np.diff(co.bounds(c["chr_pos"], c["x"].shape[1]))
    assert info["n_chromosomes"] == len(c["chr_pos"]) and info["longest_chromosome"] == int(lengths.max())
    assert set(info["stage_ms"]) == {"sigma", "levels"}


def test_the_cases_cover_what_they_are_named_for():
    assert co.expected("beta_0")["want"]["beta"] == 0.0
    assert co.expected("beta_huge")["want"]["n_segments"].tolist() == [4, 4, 4]  # one segment per chromosome
    assert co.expected("m_is_L_plus_1")["want"]["n_segments"].tolist() == [3, 3, 3]
    assert (co.expected("m_half_L")["want"]["n_segments"] > 3).any()  # exactly two pieces of 32 fit
    assert co.expected("empty_row")["want"]["n_segments"][1] == 3 and co.expected("empty_row")["x"][1].nnz == 0
    assert int(co.expected("chromosome_4096")["want"]["starts"][0, :4096].sum()) > 10
    assert (co.expected("ties_beta_0")["want"]["n_segments"][:4] == 5).all()  # constant rows: ties keep them whole


# ---- the default sigma ---------------------------------------------------------------------------------------------------------
def test_the_sums_of_squared_differences_are_the_oracles():
    from infercnvpy_amd import _engine

    for name in ("mixed_n3", "mixed_n70", "chromosomes_70", "empty_row", "ties"):
        c = co.expected(name)
        edges = co.bounds(c["chr_pos"], c["x"].shape[1])
        want = np.asarray(co.diffsq(co.rows_of(c["x"]), edges))
        for x in (c["x"], c["x"].toarray(), c["x"].astype(np.float32)):
            ref = want if x.dtype == np.float64 else np.asarray(
                co.diffsq(co.rows_of(x.astype(np.float64)), edges))
            got = _engine.changepoint_diffsq(_engine.matrix_input(x, "test"), np.asarray(edges, dtype=np.int32)).cpu().numpy()
            assert co.same_bytes(got, ref), name


# ---- every input kind ----------------------------------------------------------------------------------------------------------
def _inputs(x):
    import torch

    import infercnvpy_amd as cnv

    def packed(tail):
        pad_i = torch.full((tail,), 2 ** 30, dtype=torch.int32)  # (never read: a column far outside the matrix, a NaN)
        pad_v = torch.full((tail,), float("nan"), dtype=torch.float64)
        return cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(),
                             torch.cat([torch.from_numpy(x.indices.astype(np.int32)), pad_i]).cuda(),
                             torch.cat([torch.from_numpy(x.data), pad_v]).cuda(), x.shape[1])

    dense = x.toarray()
    filler = np.where(np.arange(dense.size) % 2 == 0, -0.0, 0.0).reshape(dense.shape)
    return {"csr": x, "csc": x.tocsc(), "dense_c": dense, "dense_f": np.asfortranarray(dense),
            "dense_with_minus_zeros": np.where(dense == 0, filler, dense),
            "cuda_float64": torch.from_numpy(dense).cuda(), "packed_csr": packed(0), "packed_csr_with_a_tail": packed(37)}


def test_every_input_kind_gives_the_same_bytes():
    import torch

    import infercnvpy_amd as cnv

    lengths = (40, 1, 64, 30)
    x64 = co.steps(9, lengths, 31, density=0.3)
    chr_pos = co.chr_pos_of(lengths)
    for dtype in (np.float64, np.float32):
        x = x64.astype(dtype).astype(np.float64)  # (the float32 matrix, its values as the float64 the kernel uses)
        want = co.cnv_changepoints(x, chr_pos)
        kinds = _inputs(x) if dtype == np.float64 else {
            "csr_float32": x.astype(np.float32), "dense_float32": x.toarray().astype(np.float32),
            "cuda_float32": torch.from_numpy(x.toarray().astype(np.float32)).cuda()}
        for kind, given in kinds.items():
            ad = _adata(given, chr_pos)
            levels, starts, info = cnv.tl.cnv_changepoints(ad, inplace=False, return_info=True)
            assert set(ad.obsm) == {"X_cnv"} and list(ad.obs.columns) == [] and set(ad.uns) == {"cnv"}, kind
            on_device = isinstance(given, (torch.Tensor, cnv.PackedCsr))
            assert isinstance(levels, torch.Tensor if on_device else np.ndarray), kind
            if on_device:  # device input keeps the result on the device
                assert levels.is_cuda and starts.is_cuda and levels.dtype == torch.float64 and starts.dtype == torch.uint8
                levels, starts = levels.cpu().numpy(), starts.cpu().numpy()
            assert info["sigma"] == want["sigma"] and info["beta"] == want["beta"], kind
            assert_equal(levels, starts, want, kind)


def test_device_input_in_place_keeps_the_levels_on_the_device():
    import torch

    import infercnvpy_amd as cnv

    c = co.expected("empty_row")
    ad = _adata(torch.from_numpy(c["x"].toarray()).cuda(), c["chr_pos"])
    assert cnv.tl.cnv_changepoints(ad, key_added="lv") is None
    levels = ad.obsm["X_lv"]
    assert isinstance(levels, torch.Tensor) and levels.is_cuda
    assert co.same_bytes(levels.cpu().numpy(), c["want"]["levels"])
    assert ad.obs["lv_n_segments"].dtype == np.int32 and ad.obs["lv_n_segments"].tolist() == c["want"]["n_segments"].tolist()


# ---- refusals that need the device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_values_are_refused(bad):
    import infercnvpy_amd as cnv

    x = co.steps(3, (20, 10), 41).toarray()
    x[1, 7] = bad
    for given, kw in ((sp.csr_matrix(x), {}), (x, {"sigma": 0.1})):
        ad = _adata(given, {"a": 0, "b": 20})
        with pytest.raises(ValueError) as info:
            cnv.tl.cnv_changepoints(ad, **kw)
        assert info.value.args[0] == "tl.cnv_changepoints: X_cnv has non-finite values"
        assert set(ad.obsm) == {"X_cnv"} and set(ad.uns) == {"cnv"}


def test_values_that_could_overflow_are_refused():
    import infercnvpy_amd as cnv

    x = np.zeros((2, 30))
    x[0, 3] = 1e154
    with pytest.raises(ValueError, match="^tl.cnv_changepoints: the value of magnitude 1e\\+154 in X_cnv overflows float64"):
        cnv.tl.cnv_changepoints(_adata(x, {"a": 0}), sigma=0.1)
    x[0, 3] = 1.0
    with pytest.raises(ValueError, match="^tl.cnv_changepoints: penalty=1e\\+300 and sigma=1e\\+100 overflow float64"):
        cnv.tl.cnv_changepoints(_adata(x, {"a": 0}), sigma=1e100, penalty=1e300)
    with pytest.raises(ValueError, match="^tl.cnv_changepoints: the default sigma of X_cnv overflows float64; pass sigma"):
        cnv.tl.cnv_changepoints(_adata(np.tile([1e153, -1e153], (2, 15)), {"a": 0}))


# ---- the table, in place -------------------------------------------------------------------------------------------------------
def test_the_table_and_everything_written_in_place():
    import infercnvpy_amd as cnv

    c = co.expected("mixed_n3")
    want = c["want"]
    ad = _adata(c["x"], c["chr_pos"])
    assert cnv.tl.cnv_changepoints(ad) is None
    assert set(ad.obsm) == {"X_cnv", "X_cnv_levels"} and list(ad.obs.columns) == ["cnv_levels_n_segments"]
    assert co.same_bytes(ad.obsm["X_cnv_levels"], want["levels"])
    assert ad.obs["cnv_levels_n_segments"].dtype == np.int32
    assert ad.obs["cnv_levels_n_segments"].tolist() == want["n_segments"].tolist()
    out = ad.uns["cnv_levels"]
    assert set(out) == {"chr_pos", "params", "use_rep", "segments"} and out["use_rep"] == "cnv"
    assert out["chr_pos"] == c["chr_pos"] and out["chr_pos"] is not ad.uns["cnv"]["chr_pos"]
    assert out["params"] == {"penalty": 2.0, "sigma": want["sigma"], "beta": want["beta"], "min_windows": 1}
    table = out["segments"]
    assert list(table.columns) == ["cell", "chromosome", "start", "end", "n_windows", "mean"]
    assert [str(t) for t in table.dtypes] == ["int64", "object", "int32", "int32", "int32", "float64"]
    rows = list(zip(*(table[k].tolist() for k in table.columns)))
    assert rows == want["table"]  # (floats compare by value: the means are the oracle's doubles)
    assert co.same_bytes(table["mean"].to_numpy(), np.asarray([t[5] for t in want["table"]]))
    # table=False leaves the table out, and nothing else
    ad2 = _adata(c["x"], c["chr_pos"])
    cnv.tl.cnv_changepoints(ad2, table=False, key_added="lv")
    assert set(ad2.uns["lv"]) == {"chr_pos", "params", "use_rep"} and co.same_bytes(ad2.obsm["X_lv"], want["levels"])


# ---- the planted case and what composes with the result ---------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_the_planted_case_through_the_public_call(seed):
    import infercnvpy_amd as cnv

    c = co.planted(seed)
    ad = _adata(sp.csr_matrix(c["x"]), c["chr_pos"])
    levels, starts, info = cnv.tl.cnv_changepoints(ad, return_info=True)
    f = co.planted_figures(c["truth"], levels, starts)
    print(f"seed {seed}: sigma = {info['sigma']:.4f}, {f}")
    assert f["n_segments"] == co.PLANTED_SEGMENTS == len(ad.uns["cnv_levels"]["segments"])
    assert f["shift"] <= 2 and f["mean_error"] <= 0.1 and f["off"] <= 5
    assert (levels[:, 115] - levels[:, 35]).min() > 0.2
    want = co.cnv_changepoints(c["x"], c["chr_pos"])
    assert info["sigma"] == want["sigma"]
    assert_equal(levels, starts, want, seed)


def test_the_states_and_the_clone_profiles_compose_with_it():
    import infercnvpy_amd as cnv

    c = co.planted(0)
    ad = _adata(sp.csr_matrix(c["x"]), c["chr_pos"])
    ad.obs["clone"] = pd.Categorical(list("aaabbb"))
    cnv.tl.cnv_changepoints(ad)
    cnv.tl.cnv_states(ad, use_rep="cnv_levels", key_added="states_of_levels")
    states = ad.obsm["X_states_of_levels"]
    assert co.same_bytes(states, so.cnv_states(ad.obsm["X_cnv_levels"], c["chr_pos"])[0])
    assert (states[:, 105:125] == 1).all() and (states[:, 60:85] == 0).all()
    clones = cnv.tl.cnv_pseudobulk(ad, "clone")
    cnv.tl.cnv_changepoints(clones)
    want = co.cnv_changepoints(clones.obsm["X_cnv"], c["chr_pos"])
    assert co.same_bytes(clones.obsm["X_cnv_levels"], want["levels"])
    assert sorted(set(clones.uns["cnv_levels"]["segments"]["cell"])) == [0, 1]

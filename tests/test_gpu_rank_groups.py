"""tl.cnv_rank_groups on the GPU equals the oracle of DESIGN.md 4.20 (tests/_rank_oracle.py): the int64 tables R2 and T
exactly and the float64 results on the bytes, for every kind of input, at the limits of the kernels (runs of equal values
across every boundary of the rank-sum kernel, zeros of both signs, one-sided columns, extreme values, tiny populations,
as many groups as the LDS table of the rank sums holds and more, where the sums go to global atomics),
for any cut of the windows into tiles; non-finite values raise; the planted clones are found."""
import functools

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp

import _rank_oracle as ro

pytestmark = pytest.mark.gpu

CHR_POS = {"chr1": 0, "chr2": 20}
FIELDS = ("scores", "pvals", "pvals_adj", "auc")


def _adata(x, chr_pos, labels, name="clone"):
    from infercnvpy_amd._compat import SimpleAnnData

    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=pd.DataFrame({name: labels}))
    ad.obsm["X_cnv"] = x
    ad.uns["cnv"] = {"chr_pos": dict(chr_pos)}
    return ad


def _labels(codes, names):
    return pd.Categorical.from_codes(np.asarray(codes), categories=names)


@functools.lru_cache(maxsize=None)
def kinds_case():
    """67 cells x 37 windows, 4 groups, missing labels and a group of one cell; the oracle's result for min_cells=2,
    computed once."""
    x, codes = ro.random_case()
    want = ro.rank_groups(x, codes, 5, sorted(CHR_POS.values()), min_cells=2)
    assert want["kept"].tolist() == [0, 1, 2, 3] and want["N"] == int((codes >= 0).sum()) < 67
    assert (want["T"] > 0).all() and (want["pvals"] < 1).any()
    return {"x": x, "codes": codes, "labels": _labels(codes, list("abcde")), "want": want}


def _inputs(x):
    import torch

    import infercnvpy_amd as cnv

    dense32 = x.toarray().astype(np.float32)
    packed = cnv.PackedCsr(torch.from_numpy(x.indptr.astype(np.int64)).cuda(), torch.from_numpy(x.indices.astype(np.int32)).cuda(),
                           torch.from_numpy(x.data).cuda(), x.shape[1])
    return {"csr": x, "csr_float32": x.astype(np.float32), "csc": x.tocsc(), "dense_float32": dense32,
            "dense_float64": dense32.astype(np.float64), "cuda_float32": torch.from_numpy(dense32).cuda(),
            "cuda_float64": torch.from_numpy(dense32.astype(np.float64)).cuda(), "packed_csr": packed}


def _tables(x, code, n_groups, **kw):
    """(R2, T) of the engine binding as host int64 arrays for the oracle's kind of code."""
    from infercnvpy_amd import _engine

    code = np.asarray(code, dtype=np.int64)
    code = np.where(code >= n_groups, n_groups, code)
    n_cells = np.bincount(code[(code >= 0) & (code < n_groups)], minlength=n_groups).astype(np.int64)
    dm = _engine.matrix_input(x, "test")
    r2, tie, bits = _engine.rank_tables(dm, code.astype(np.int32), n_cells, **kw)
    assert bits == 0
    return r2.cpu().numpy(), tie.cpu().numpy(), n_cells


def _same_regions(table, want, labels, n_cells):
    assert list(table.columns) == ["group", "chromosome", "start", "end", "direction", "n_windows", "n_cells", "score",
                                   "pvals_adj_max", "auc"]
    assert len(table) == len(want)
    for row, (g, a, b, d, score, worst, mean_auc) in zip(table.itertuples(index=False), want):
        assert (row.group, row.start, row.end, row.direction, row.n_windows, row.n_cells) == (labels[g], a, b, d, b - a, n_cells[g])
        assert (row.score, row.pvals_adj_max, row.auc) == (score, worst, mean_auc)


# ---- the bytes for every input kind ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["csr", "csr_float32", "csc", "dense_float32", "dense_float64", "cuda_float32", "cuda_float64",
                                  "packed_csr"])
def test_every_input_kind_gives_the_oracles_integers_and_bytes(kind):
    import infercnvpy_amd as cnv
    from infercnvpy_amd import _engine

    c = kinds_case()
    want = c["want"]
    x = _inputs(c["x"])[kind]
    r2, tie, bits = _engine.rank_tables(_engine.matrix_input(x, "test"), want["code"].astype(np.int32), want["n_cells"])
    assert bits == 0 and r2.dtype == tie.dtype and str(r2.dtype) == "torch.int64"
    assert (r2.cpu().numpy() == want["R2"]).all() and (tie.cpu().numpy() == want["T"]).all()

    ad = _adata(x, CHR_POS, c["labels"])
    assert cnv.tl.cnv_rank_groups(ad, "clone") is None
    got = ad.uns["cnv_rank_groups"]
    assert set(got) == {"groups", "n_cells", "scores", "pvals", "pvals_adj", "auc", "mean", "chr_pos", "params", "dropped",
                        "regions"}
    for name in FIELDS + ("mean",):
        assert isinstance(got[name], np.ndarray) and got[name].dtype == np.float64 and got[name].shape == (4, 37), name
    for name in FIELDS:
        assert got[name].tobytes() == want[name].tobytes(), name
    assert list(got["groups"]) == list("abcd") and got["dropped"] == ["e"]
    assert got["n_cells"].dtype == np.int64 and got["n_cells"].tolist() == want["n_cells"].tolist()
    assert got["chr_pos"] == CHR_POS and got["chr_pos"] is not ad.uns["cnv"]["chr_pos"]
    assert got["params"] == {"groupby": "clone", "use_rep": "cnv", "min_cells": 2, "alpha": 0.05, "min_windows": 1,
                             "n_population": want["N"]}
    _same_regions(got["regions"], want["regions"], list("abcd"), want["n_cells"])
    assert ad.obsm["X_cnv"] is x  # the matrix is not touched


def test_the_means_are_those_of_cnv_pseudobulk_and_the_other_arguments_act():
    import infercnvpy_amd as cnv

    c = kinds_case()
    ad = _adata(c["x"], CHR_POS, c["labels"])
    out, info = cnv.tl.cnv_rank_groups(ad, "clone", inplace=False, return_info=True, alpha=0.5, min_windows=2, min_cells=1,
                                       key_added="other")
    assert "other" not in ad.uns and "cnv_rank_groups" not in ad.uns
    clones = cnv.tl.cnv_pseudobulk(ad, "clone", min_cells=1)
    assert out["mean"].tobytes() == np.asarray(clones.X).tobytes() and list(out["groups"]) == list("abcde")
    want = ro.rank_groups(c["x"], c["codes"], 5, sorted(CHR_POS.values()), min_cells=1, alpha=0.5, min_windows=2)
    for name in FIELDS:
        assert out[name].tobytes() == want[name].tobytes(), name
    assert len(want["regions"]) > 0 and all(b - a >= 2 for _, a, b, *_ in want["regions"])
    _same_regions(out["regions"], want["regions"], list("abcde"), want["n_cells"])
    assert info["n_groups"] == 5 and info["n_tiles"] == 1 and info["n_entries"] == int(want["N"] * 37 - _zeros(c, want))
    assert set(info["stage_ms"]) == {"tables", "means", "finish", "count", "scatter", "sort", "rank_sums", "finish_kernel"}
    # inplace under another key, for a plain label column
    plain = np.where(c["codes"] < 0, None, c["codes"].astype(object))
    ad = _adata(c["x"].toarray(), CHR_POS, plain, name="cnv_leiden")
    assert cnv.tl.cnv_rank_groups(ad, key_added="mine") is None and set(ad.uns) == {"cnv", "mine"}
    codes2, uniques = pd.factorize(plain, use_na_sentinel=True)
    want = ro.rank_groups(c["x"], codes2, len(uniques), sorted(CHR_POS.values()))
    assert ad.uns["mine"]["scores"].tobytes() == want["scores"].tobytes()
    assert list(ad.uns["mine"]["groups"]) == list(uniques[want["kept"]])


def _zeros(c, want):
    pop = ro.dense_rows(c["x"])[want["code"] >= 0]
    return int((pop == 0).sum())


# ---- the limits ------------------------------------------------------------------------------------------------------------
LIMITS = ro.limit_cases()


@pytest.mark.parametrize("name", [c[0] for c in LIMITS])
def test_limits_equal_the_oracle(name):
    (_, x, code, n_groups), = [c for c in LIMITS if c[0] == name]
    want_r2, want_tie, flags = ro.tables(x, code, n_groups)
    assert flags == 0
    r2, tie, n_cells = _tables(x, code, n_groups)
    assert (r2 == want_r2).all() and (tie == want_tie).all(), name
    n_pop = int((np.asarray(code) >= 0).sum())
    if n_cells.sum() == n_pop:  # every ranked cell is in a tested group: the doubled ranks 1 .. N
        assert (r2.sum(axis=0) == n_pop * (n_pop + 1)).all()
    # the finish of the package on these tables: the degenerate rule where it applies, the oracle's bytes everywhere
    from infercnvpy_amd.tl import _rank

    z, p, auc = _rank.rank_statistics(r2, tie, n_cells, n_pop)
    wz, wp, wauc = ro.statistics(want_r2, want_tie, n_cells, n_pop)
    assert z.tobytes() == wz.tobytes() and p.tobytes() == wp.tobytes() and auc.tobytes() == wauc.tobytes()
    assert np.isfinite(z).all() and np.isfinite(p).all() and np.isfinite(auc).all()
    if name in ("one_group_is_the_population", "one_cell", "one_cell_among_unlabelled"):
        assert (z == 0).all() and (p == 1).all() and (auc == 0.5).all()


def test_the_limit_cases_hold_what_they_are_for():
    """The properties of the inputs that make a wrong kernel fail on them (checked on the host)."""
    by_name = {c[0]: c for c in LIMITS}
    # a stored -0.0 that would rank below every zero if its sign bit were read: the tables differ from those of a column
    # where it is a negative value
    _, x, code, g = by_name["minus_zero_is_no_negative"]
    as_negative = x.copy()
    as_negative.data[np.signbit(as_negative.data) & (as_negative.data == 0)] = -1e-300
    assert (ro.tables(x, code, g)[0] != ro.tables(as_negative, code, g)[0]).any()
    # runs of equal values that cover sorted positions on both sides of a multiple of 64, of 256 and of 2048
    _, x, _, _ = by_name["runs_at_wave_and_workgroup_boundaries"]
    crossed = set()
    for j in range(x.shape[1]):
        col = np.sort(x[:, j])
        s = int(np.searchsorted(col, 2.0, side="left"))
        e = int(np.searchsorted(col, 2.0, side="right"))
        crossed |= {b for b in (ro.WAVE, ro.SUM_THREADS, 2 * ro.SUM_THREADS, 1024) if s < b < e}
        crossed |= {("starts at", b) for b in (0, ro.WAVE, ro.SUM_THREADS) if s == b}
    assert {ro.WAVE, ro.SUM_THREADS, 2 * ro.SUM_THREADS, 1024, ("starts at", 0)} <= crossed
    assert sorted({int((x[:, j] == 2.0).sum()) for j in range(x.shape[1])}) == [63, 64, 65, 255, 256, 257, 1025]
    _, x, _, _ = by_name["runs_at_the_chunk_boundary"]
    assert x.shape[0] > ro.CHUNK
    for j in range(x.shape[1]):
        col = np.sort(x[:, j])
        assert np.searchsorted(col, 2.0, side="left") < ro.CHUNK < np.searchsorted(col, 2.0, side="right")
    _, x, _, _ = by_name["rows_of_200_entries"]
    assert np.diff(x.indptr).max() > 2 * ro.WAVE
    # the codes at and past the LDS table of the rank sums: G tested groups and the code G of the cells in none of them
    for name, fills in (("groups_fill_the_lds_table", True), ("groups_one_past_the_lds_table", False),
                        ("groups_far_past_the_lds_table", False)):
        _, x, code, g = by_name[name]
        assert (g + 1 == ro.LDS_GROUPS) if fills else (g + 1 > ro.LDS_GROUPS)
        n_pop = int((code >= 0).sum())
        assert x.shape[0] >= n_pop > ro.CHUNK and (x[code >= 0, 0] != 0).all()  # window 0: a segment of two chunks
        sizes = np.bincount(code[(code >= 0) & (code < g)], minlength=g)
        assert sizes.min() >= 1 and sizes.max() > 2 and int(code.max()) == g and 90 <= int((code == g).sum()) <= 110
        col = np.sort(x[code >= 0, 1])
        assert np.searchsorted(col, 2.0, side="left") < ro.CHUNK < np.searchsorted(col, 2.0, side="right")
    assert by_name["groups_one_past_the_lds_table"][3] == ro.LDS_GROUPS
    assert (by_name["groups_far_past_the_lds_table"][2] == -1).sum() == 5


# ---- tiles -------------------------------------------------------------------------------------------------------------------
def test_any_cut_into_window_tiles_gives_the_same_tables():
    c = kinds_case()
    want = c["want"]
    for x in (c["x"], c["x"].toarray()):
        info = {}
        # max_entries is never below the population: force the population down by ranking 12 cells only
        code = np.where(np.arange(67) < 12, np.maximum(want["code"], 0), -1)
        want_r2, want_tie, _ = ro.tables(c["x"], code, 4)
        r2, tie, _ = _tables(x, code, 4, max_entries=1, info=info)
        assert info["n_tiles"] >= 3 and (r2 == want_r2).all() and (tie == want_tie).all()
        whole = {}
        r2, tie, _ = _tables(x, code, 4, info=whole)
        assert whole["n_tiles"] == 1 and whole["n_entries"] == info["n_entries"]
        assert (r2 == want_r2).all() and (tie == want_tie).all()
    # the whole population, the tightest budget: one tile per window that stores anything
    info = {}
    r2, tie, _ = _tables(c["x"], want["code"], 4, max_entries=1, info=info)
    assert info["n_tiles"] >= 3 and (r2 == want["R2"]).all() and (tie == want["T"]).all()


def test_window_tiles_feed_the_same_global_tables_past_the_lds_table():
    """G + 1 = 2049 codes: every tile's rank sums go to the global tables entry by entry, and the tiles add up."""
    (_, x, code, g), = [c for c in LIMITS if c[0] == "groups_one_past_the_lds_table"]
    want_r2, want_tie, _ = ro.tables(x, code, g)
    info = {}
    r2, tie, _ = _tables(x, code, g, max_entries=1, info=info)
    assert info["n_tiles"] >= 3 and (r2 == want_r2).all() and (tie == want_tie).all()


# ---- non-finite input ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("dense", [False, True])
def test_a_non_finite_value_raises(value, dense):
    import infercnvpy_amd as cnv

    c = kinds_case()
    x = c["x"].copy()
    row = int(np.flatnonzero(c["codes"] >= 0)[3])
    x.data[x.indptr[row]] = value
    ad = _adata(x.toarray() if dense else x, CHR_POS, c["labels"])
    with pytest.raises(ValueError) as info:
        cnv.tl.cnv_rank_groups(ad, "clone")
    assert info.value.args[0] == "tl.cnv_rank_groups: X_cnv has non-finite values"
    assert "cnv_rank_groups" not in ad.uns


def test_a_non_finite_value_of_a_cell_without_a_label_is_not_read_by_the_ranking():
    from infercnvpy_amd import _engine

    c = kinds_case()
    x = c["x"].copy()
    row = int(np.flatnonzero(c["codes"] < 0)[0])
    x.data[x.indptr[row]] = np.nan
    want = c["want"]
    r2, tie, bits = _engine.rank_tables(_engine.matrix_input(x, "test"), want["code"].astype(np.int32), want["n_cells"])
    assert bits == 0 and (r2.cpu().numpy() == want["R2"]).all() and (tie.cpu().numpy() == want["T"]).all()


# ---- the planted clones ----------------------------------------------------------------------------------------------------
def test_planted_clones():
    import infercnvpy_amd as cnv

    x, codes, truth = ro.planted_clones(0)
    want = ro.rank_groups(x, codes, 4, sorted(ro.PLANTED_CHR.values()))
    ad = _adata(sp.csr_matrix(x), ro.PLANTED_CHR, _labels(codes, ["clone0", "clone1", "clone2", "normal"]))
    out = cnv.tl.cnv_rank_groups(ad, "clone", inplace=False)
    for name in FIELDS:
        assert out[name].tobytes() == want[name].tobytes(), name
    _same_regions(out["regions"], want["regions"], ["clone0", "clone1", "clone2", "normal"], want["n_cells"])
    missed, false_calls = ro.planted_verdict(want, truth)
    print(f"{missed} of 75 planted pairs missed or wrong-signed, {false_calls} event-free calls of 780")
    assert missed == 0 and false_calls <= 8
    table = out["regions"]
    for label, a, b, d in (("clone0", 20, 50, 1), ("clone1", 100, 130, -1), ("clone2", 200, 210, 1), ("clone2", 210, 215, 1)):
        hit = table[(table["group"] == label) & (table["start"] <= a) & (table["end"] >= b)]
        assert len(hit) == 1 and int(hit["direction"].iloc[0]) == d, (label, a, b)
    clone2 = table[(table["group"] == "clone2") & (table["start"] >= 200) & (table["end"] <= 215)]
    assert clone2[["chromosome", "start", "end"]].values.tolist() == [["chr3", 200, 210], ["chr4", 210, 215]]

"""The oracle of tl.cnv_rank_groups (tests/_rank_oracle.py) against scipy's ranks and scipy's own
Mann-Whitney test, its degenerate rule and its Benjamini-Hochberg step against direct restatements, the package's host
finish against the oracle on the bytes, and everything tl.cnv_rank_groups and its entry points refuse before they touch
the device.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import scipy.stats

import _rank_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest relative deviation of the oracle's z from scipy.stats.mannwhitneyu(use_continuity=False,
# method="asymptotic") over scipy_cases() was measured at 3.03e-16 (scipy 1.15.3: it forms the same quantities in another
# order -- U - n1 n2 / 2 in floats, the tie term divided before it is subtracted); ten times that is the rounding-order
# margin asserted here.
Z_MEASURED = 3.03e-16
Z_MARGIN = 10 * Z_MEASURED


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def scipy_cases():
    """5 seeds of 60 cells x 40 windows: thresholded normal values in 3 groups (a matrix like X_cnv: most of a column is
    one tie), plus the random case of the GPU test."""
    cases = []
    for seed in range(5):
        rng = np.random.default_rng(seed)
        x = rng.normal(0.0, 0.3, (60, 40))
        x[np.abs(x) < 0.15] = 0.0
        cases.append((x, rng.integers(0, 3, size=60), 3))
    x, codes = ro.random_case()
    cases.append((x, codes, 5))
    return cases


# ---- rule 2 against scipy's ranks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(6))
def test_doubled_rank_sums_equal_twice_scipys_average_ranks(case):
    x, codes, n_groups = scipy_cases()[case]
    code, kept, n_cells, n_pop = ro.population(codes, n_groups, 1)
    r2, tie, flags = ro.tables(x, code, len(kept))
    assert flags == 0 and r2.dtype == np.int64 and tie.dtype == np.int64
    pop = ro.dense_rows(x)[code >= 0]
    ranks2 = 2.0 * scipy.stats.rankdata(pop, method="average", axis=0)  # (halves: exact in float64)
    assert (ranks2 == np.rint(ranks2)).all()
    group = code[code >= 0]
    for g in range(len(kept)):
        assert (r2[g] == ranks2[group == g].sum(axis=0).astype(np.int64)).all()
    assert (r2.sum(axis=0) == n_pop * (n_pop + 1)).all()  # every cell is in a tested group here: the ranks 1 .. N, doubled
    for j in range(pop.shape[1]):
        _, c = np.unique(pop[:, j], return_counts=True)
        assert int(tie[j]) == int((c.astype(np.int64) ** 3 - c).sum())


@pytest.mark.parametrize("case", range(3))
def test_the_cases_at_the_lds_table_equal_twice_scipys_average_ranks(case):
    """The oracle's tables of the three cases with about 2 048 groups (tests/test_gpu_rank_groups.py compares the kernels
    with them) against scipy's ranks, and what the cases are built to hold."""
    name, x, code, g = ro.lds_table_cases()[case]
    assert name == ("groups_fill_the_lds_table", "groups_one_past_the_lds_table", "groups_far_past_the_lds_table")[case]
    assert x.shape == (ro.LDS_TABLE_CELLS, 5) and x.dtype == np.float64 and code.shape == (x.shape[0],)
    assert g + 1 == (ro.LDS_GROUPS, ro.LDS_GROUPS + 1, 2201)[case] and int(code.max()) == g
    assert int((code == -1).sum()) == (0, 0, 5)[case] and int(code.min()) == (0, 0, -1)[case]
    n_pop = int((code >= 0).sum())
    assert n_pop > ro.CHUNK
    sizes = np.bincount(code[(code >= 0) & (code < g)], minlength=g)
    assert sizes.min() >= 1 and sizes.max() > 2
    pop, group = x[code >= 0], code[code >= 0]
    assert (pop[:, 0] != 0).all() and 0.3 < (pop[:, 2] != 0).mean() < 0.5 and (pop[:, 2] < 0).any() and (pop[:, 2] > 0).any()
    assert (pop[:, 3] == 0).all() and (pop[:, 4] < 0).all()
    r2, tie, flags = ro.tables(x, code, g)
    assert flags == 0 and r2.shape == (g, 5)
    ranks2 = 2.0 * scipy.stats.rankdata(pop, method="average", axis=0)
    want = np.zeros((g + 1, 5), dtype=np.int64)
    np.add.at(want, group, ranks2.astype(np.int64))
    assert (ranks2 == np.rint(ranks2)).all() and (r2 == want[:g]).all()
    assert (r2.sum(axis=0) + want[g] == n_pop * (n_pop + 1)).all() and (want[g] > 0).all()  # the untested cells hold ranks
    run = int((pop[:, 1] == 2.0).sum())  # (the run ends with the column: what of the 1 025 fits behind CHUNK - 500 values)
    assert run > 700 and tie[0] == 0 and tie[1] == run ** 3 - run and tie[3] == n_pop ** 3 - n_pop and tie[2] > 0


def test_a_stored_minus_zero_is_the_zero_and_dropped_groups_stay_in_the_rest():
    x = sp.csr_matrix((np.asarray([-0.0, 0.0, -0.0, 2.0]), np.asarray([0, 0, 0, 0]), np.asarray([0, 1, 2, 3, 4])), shape=(4, 1))
    r2, tie, _ = ro.tables(x, np.asarray([0, 1, 0, 1]), 2)
    # three zeros share the mid-rank 2 (doubled 4), the 2.0 has rank 4 (doubled 8); one tie of three: 27 - 3
    assert r2.tolist() == [[8], [12]] and tie.tolist() == [24]
    # group 1 below min_cells: its cells are ranked (code 1 = the pseudo-group of one tested group) but not summed
    code, kept, n_cells, n_pop = ro.population(np.asarray([0, 1, 0, 0, -1]), 2, 2)
    assert code.tolist() == [0, 1, 0, 0, -1] and kept.tolist() == [0] and n_cells.tolist() == [3] and n_pop == 4
    r2, tie, _ = ro.tables(np.asarray([[1.0], [5.0], [2.0], [9.0], [7.0]]), code, 1)
    assert r2.tolist() == [[2 * (1 + 2 + 4)]] and tie.tolist() == [0]  # (the unlabelled 7.0 is not ranked)


# ---- rule 3 against scipy's test -------------------------------------------------------------------------------------------
def test_z_p_and_auc_agree_with_scipys_mannwhitneyu_within_the_measured_margin():
    worst_z = worst_p = worst_auc = 0.0
    erfc_ulps = 8 * 2.0 ** -52  # what two implementations of the normal tail may differ by on one argument
    for x, codes, n_groups in scipy_cases():
        res = ro.rank_groups(x, codes, n_groups, [0], min_cells=2)
        pop, group = ro.dense_rows(x)[res["code"] >= 0], res["code"][res["code"] >= 0]
        for g in range(len(res["kept"])):
            a, b = pop[group == g], pop[group != g]
            for j in range(pop.shape[1]):
                if np.ptp(pop[:, j]) == 0:
                    continue  # (the degenerate rule: scipy divides by 0 there)
                want = scipy.stats.mannwhitneyu(a[:, j], b[:, j], use_continuity=False, method="asymptotic")
                n1, n2 = a.shape[0], b.shape[0]
                mu = n1 * n2 / 2.0
                tie_term = float(res["T"][j]) / (res["N"] * (res["N"] - 1.0))
                want_z = (want.statistic - mu) / np.sqrt(n1 * n2 / 12.0 * ((res["N"] + 1) - tie_term))
                z, p, auc = res["scores"][g, j], res["pvals"][g, j], res["auc"][g, j]
                if want_z != 0.0:
                    worst_z = max(worst_z, abs(z - want_z) / abs(want_z))
                else:
                    assert z == 0.0
                # p = erfc(|z| / sqrt(2)) = 2 Q(|z|): |d ln p / d ln z| = z phi(z) / Q(z) <= z^2 + 1 (Mills' ratio), and scipy's
                # p comes from its own z
                assert abs(p - want.pvalue) / want.pvalue <= (z * z + 1.0) * Z_MARGIN + erfc_ulps, (g, j, p, want.pvalue)
                worst_p = max(worst_p, abs(p - want.pvalue) / want.pvalue)
                worst_auc = max(worst_auc, abs(auc - want.statistic / (n1 * n2)))
    print(f"largest relative deviation: z {worst_z:.3e}, p {worst_p:.3e}; largest absolute deviation of auc {worst_auc:.3e}")
    assert 0.0 < worst_z <= Z_MARGIN
    assert worst_auc <= 2.0 ** -52  # U / (n1 n2): one division here, one there


def test_degenerate_rule():
    # an all-equal column: k = 0
    x = np.full((6, 2), 0.25)
    x[:, 1] = 0.0
    res = ro.rank_groups(x, np.asarray([0, 0, 1, 1, 1, 1]), 2, [0], min_cells=1)
    assert (res["T"] == 6 ** 3 - 6).all() and (res["scores"] == 0.0).all() and (res["pvals"] == 1.0).all()
    assert (res["auc"] == 0.5).all() and (res["pvals_adj"] == 1.0).all() and res["regions"] == []
    # one group that covers the population: n2 = 0
    x = np.asarray([[1.0, 0.0], [2.0, 0.0], [3.0, 1.0]])
    res = ro.rank_groups(x, np.zeros(3, dtype=np.int64), 1, [0], min_cells=1)
    assert (res["scores"] == 0.0).all() and (res["pvals"] == 1.0).all() and (res["auc"] == 0.5).all()
    # and one cell
    res = ro.rank_groups(np.asarray([[0.5, 0.0, -1.0]]), np.zeros(1, dtype=np.int64), 1, [0], min_cells=1)
    assert res["R2"].tolist() == [[2, 2, 2]] and (res["scores"] == 0.0).all() and (res["auc"] == 0.5).all()


def test_benjamini_hochberg_against_a_direct_restatement():
    rng = np.random.default_rng(0)
    p = rng.random((4, 23)) ** 3
    p[1, 5] = p[1, 9] = p[1, 2]  # equal p-values: the stable sort decides, the result does not depend on it
    p[2, :] = 1.0
    p[3, 0] = 0.0
    got = ro.adjust(p)
    for g in range(4):
        for j in range(23):
            # the smallest p_(k) W / k over the ranks k from this p's rank on = over the p-values at or above it
            want = min(min(1.0, pk * 23.0 / k) for k, pk in enumerate(np.sort(p[g]), start=1) if pk >= p[g, j])
            assert got[g, j] == want
    assert (got >= p).all() and (got <= 1.0).all()
    statsmodels_example = ro.adjust(np.asarray([[0.01, 0.04, 0.03, 0.005]]))
    assert np.allclose(statsmodels_example, [[0.02, 0.04, 0.04, 0.02]], rtol=1e-15)


def test_the_package_finishes_with_the_oracles_bytes():
    from infercnvpy_amd.tl import _rank

    for x, codes, n_groups in scipy_cases() + [(np.full((6, 2), 0.25), np.asarray([0, 0, 1, 1, 1, 1]), 2),
                                               (np.asarray([[0.5, 0.0, -1.0]]), np.zeros(1, dtype=np.int64), 1)]:
        res = ro.rank_groups(x, codes, n_groups, [0], min_cells=1)
        z, p, auc = _rank.rank_statistics(res["R2"], res["T"], res["n_cells"], res["N"])
        assert (bits(z) == bits(res["scores"])).all() and (bits(p) == bits(res["pvals"])).all()
        assert (bits(auc) == bits(res["auc"])).all()
        assert (bits(_rank.benjamini_hochberg(p)) == bits(res["pvals_adj"])).all()
        code, kept, _, _ = ro.population(codes, n_groups, 1)
        assert (_rank.population_codes(np.asarray(codes, dtype=np.int64), kept, n_groups) == code).all()
    code, kept, _, _ = ro.population(np.asarray([0, 1, 0, 2, -1, 2]), 4, 2)  # group 1 too small, group 3 unused
    assert code.tolist() == [0, 2, 0, 1, -1, 1]
    assert _rank.population_codes(np.asarray([0, 1, 0, 2, -1, 2]), kept, 4).tolist() == code.tolist()


def test_window_tiles_cover_the_windows_within_the_budget():
    from infercnvpy_amd import _engine

    counts = np.asarray([5, 0, 7, 7, 1, 0, 0, 9, 2], dtype=np.int64)
    assert _engine.rank_window_tiles(counts, 1 << 28) == [(0, 9)]
    assert _engine.rank_window_tiles(counts, 9) == [(0, 2), (2, 3), (3, 7), (7, 8), (8, 9)]
    assert _engine.rank_window_tiles(counts, 14) == [(0, 3), (3, 7), (7, 9)]
    assert _engine.rank_window_tiles(np.zeros(4, dtype=np.int64), 3) == [(0, 4)]
    # a window above the budget is a tile of its own (the binding never lets the budget fall below the population)
    assert _engine.rank_window_tiles(counts, 1) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 7), (7, 8), (8, 9)]


# ---- the planted clones ---------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
def test_planted_clones_are_found_with_few_event_free_calls(seed):
    x, codes, truth = ro.planted_clones(seed)
    assert int((truth != 0).sum()) == 75 and int(4 * (~(truth != 0).any(axis=0)).sum()) == 780
    res = ro.rank_groups(x, codes, 4, sorted(ro.PLANTED_CHR.values()))
    missed, false_calls = ro.planted_verdict(res, truth)
    print(f"seed {seed}: {missed} of 75 planted pairs missed or wrong-signed, {false_calls} event-free calls of 780")
    assert missed == 0 and false_calls <= 8
    found = {(g, a, b, d) for g, a, b, d, *_ in res["regions"]}
    for g, a, b, d in ((0, 20, 50, 1), (1, 100, 130, -1), (2, 200, 210, 1), (2, 210, 215, 1)):
        assert any(fg == g and fd == d and fa <= a and fb >= b for fg, fa, fb, fd in found), (g, a, b)
    assert not any(fa < 210 < fb for _, fa, fb, _ in found)  # no region crosses the chromosome start at 210


# ---- what tl.cnv_rank_groups refuses before it touches the device --------------------------------------------------------------
def _adata(n=6, w=10, x=None, chr_pos=None, labels=None):
    from infercnvpy_amd._compat import SimpleAnnData

    labels = list("aabbcc")[:n] if labels is None else labels
    ad = SimpleAnnData(np.zeros((n, 3), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))
    ad.obsm["X_cnv"] = sp.csr_matrix(np.ones((n, w))) if x is None else x
    ad.uns["cnv"] = {"chr_pos": {"chr1": 0, "chr2": 4} if chr_pos is None else chr_pos}
    return ad


def _no_chr_pos():
    ad = _adata()
    del ad.uns["cnv"]["chr_pos"]
    return ad


def _too_many_cells():
    n = 1 << 21
    return _adata(n=n, x=sp.csr_matrix((n, 1), dtype=np.float32), chr_pos={"chr1": 0}, labels=np.arange(n) % 2)


W = "tl.cnv_rank_groups: "
BAD = [
    ("missing obsm key", _adata, {"use_rep": "other"}, KeyError, W + "X_other not found in adata.obsm. Did you run `tl.infercnv`?"),
    ("missing chr_pos", _no_chr_pos, {}, KeyError, W + "chr_pos not found in adata.uns['cnv']. Did you run `tl.infercnv`?"),
    ("missing groupby", _adata, {"groupby": "nope"}, KeyError, W + "`nope` not found in `adata.obs`"),
    ("missing cnv_leiden", _adata, {"groupby": "cnv_leiden"}, KeyError,
     W + "`cnv_leiden` not found in `adata.obs`. Did you run `tl.leiden`?"),
    ("1-D X", lambda: _adata(x=np.ones(6)), {}, ValueError, W + "X_cnv must be 2-D"),
    ("empty shape", lambda: _adata(x=np.ones((6, 0))), {}, ValueError, W + "empty matrix of shape (6, 0)"),
    ("min_cells=0", _adata, {"min_cells": 0}, ValueError, W + "min_cells=0 must be an integer >= 1"),
    ("min_cells=True", _adata, {"min_cells": True}, ValueError, W + "min_cells=True must be an integer >= 1"),
    ("min_cells=1.5", _adata, {"min_cells": 1.5}, ValueError, W + "min_cells=1.5 must be an integer >= 1"),
    ("alpha=0", _adata, {"alpha": 0}, ValueError, W + "alpha=0 must be a number in (0, 1]"),
    ("alpha=1.5", _adata, {"alpha": 1.5}, ValueError, W + "alpha=1.5 must be a number in (0, 1]"),
    ("alpha=nan", _adata, {"alpha": float("nan")}, ValueError, W + "alpha=nan must be a number in (0, 1]"),
    ("alpha='x'", _adata, {"alpha": "x"}, ValueError, W + "alpha='x' must be a number in (0, 1]"),
    ("alpha=True", _adata, {"alpha": True}, ValueError, W + "alpha=True must be a number in (0, 1]"),
    ("min_windows=0", _adata, {"min_windows": 0}, ValueError, W + "min_windows=0 must be an integer >= 1"),
    ("chr_pos outside", lambda: _adata(chr_pos={"chr1": 0, "chr2": 10}), {}, ValueError,
     W + "chr_pos start 10 is outside [0, 10)"),
    ("chr_pos not at 0", lambda: _adata(chr_pos={"chr1": 1}), {}, ValueError, W + "no chromosome of chr_pos starts at window 0"),
    ("chr_pos empty", lambda: _adata(chr_pos={}), {}, ValueError, W + "chr_pos is empty"),
    ("labels of another length", lambda: _adata(x=np.ones((5, 10))), {}, ValueError,
     W + "`clone` has 6 labels for the 5 rows of X_cnv"),
    ("every group dropped", _adata, {"min_cells": 3}, ValueError, W + "no group of `clone` has min_cells=3 cells"),
    ("2^21 cells", _too_many_cells, {}, ValueError,
     W + "2097152 cells have a label; at most 2097151 are ranked against each other (N^3 in an int64)"),
]


@pytest.mark.parametrize("cid, make, kw, kind, message", BAD, ids=[c[0] for c in BAD])
def test_every_bad_input_has_its_exception_and_its_whole_message(cid, make, kw, kind, message):
    import infercnvpy_amd as cnv

    kw = {"groupby": "clone", **kw}
    with pytest.raises(kind) as info:
        cnv.tl.cnv_rank_groups(make(), **kw)
    assert type(info.value) is kind and info.value.args[0] == message


# ---- the library and the package, as far as they go without a GPU -----------------------------------------------------------
ENTRIES = ("icv_rank_count", "icv_rank_scatter", "icv_rank_sort", "icv_rank_sums", "icv_rank_finish")


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
    assert callable(_engine.rank_tables) and _engine.RANK_STAGES == ("count", "scatter", "sort", "rank_sums", "finish")
    assert "cnv_rank_groups" in cnv.tl.__all__ and callable(cnv.tl.cnv_rank_groups)
    source = open(os.path.join(ROOT, "infercnvpy_amd", "csrc", "icv_rank.hpp")).read()
    for name, value in (("kRkSumThreads", ro.SUM_THREADS), ("kRkChunk", ro.CHUNK), ("kRkSlab", ro.SLAB),
                        ("kRkTile", ro.TILE), ("kRkLdsGroups", ro.LDS_GROUPS)):
        assert f"{name} = {value};" in source  # (the sizes the limit cases are built around)
    assert f"#define ICV_RANK_MAX_CELLS (1 << 21)" in header and _lib.ICV_RANK_MAX_CELLS == ro.MAX_CELLS == 1 << 21


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from infercnvpy_amd import _lib

    lib = _lib.load()
    one = ctypes.c_void_p(8)  # never dereferenced: the arguments are refused first
    bad = _lib.ICV_ERR_INVALID
    m = _lib.Matrix()
    m.format, m.dtype, m.n_rows, m.n_cols, m.ld, m.values = _lib.ICV_DENSE, _lib.ICV_F64, 4, 5, 5, 8
    ref = ctypes.byref(m)
    big = 1 << 21

    count = lib.icv_rank_count
    assert count(None, one, one, one, None) == bad
    assert count(ref, None, one, one, None) == bad
    assert count(ref, one, None, one, None) == bad
    assert count(ref, one, one, None, None) == bad
    scatter = lib.icv_rank_scatter
    assert scatter(None, one, 0, 5, one, one, one, one, None) == bad
    assert scatter(ref, None, 0, 5, one, one, one, one, None) == bad
    assert scatter(ref, one, -1, 5, one, one, one, one, None) == bad
    assert scatter(ref, one, 0, 0, one, one, one, one, None) == bad
    assert scatter(ref, one, 1, 5, one, one, one, one, None) == bad  # (the tile ends behind the last window)
    assert scatter(ref, one, 0, 5, None, one, one, one, None) == bad
    assert scatter(ref, one, 0, 5, one, None, one, one, None) == bad
    assert scatter(ref, one, 0, 5, one, one, None, one, None) == bad
    assert scatter(ref, one, 0, 5, one, one, one, None, None) == bad
    for entry, args in ((count, (ref, one, one, one, None)), (scatter, (ref, one, 0, 1, one, one, one, one, None))):
        for field, value in (("n_cols", 0), ("n_rows", -1), ("dtype", 7), ("format", 7), ("ld", 4)):
            keep = getattr(m, field)
            setattr(m, field, value)
            assert entry(*args) == bad, field
            setattr(m, field, keep)
    assert b"rank_scatter" in lib.icv_last_error()
    sort = lib.icv_rank_sort
    assert sort(None, one, 3, one, 1, one, one, None) == bad
    assert sort(one, None, 3, one, 1, one, one, None) == bad
    assert sort(one, one, -1, one, 1, one, one, None) == bad
    assert sort(one, one, 1 << 31, one, 1, one, one, None) == bad
    assert sort(one, one, 3, None, 1, one, one, None) == bad
    assert sort(one, one, 3, one, 0, one, one, None) == bad
    assert sort(one, one, 3, one, 1, None, one, None) == bad
    assert sort(one, one, 3, one, 1, one, None, None) == bad
    assert sort(None, None, 0, one, 1, None, None, None) == _lib.ICV_OK  # no entries: nothing runs
    sums = lib.icv_rank_sums
    good = [one, one, one, 0, 5, 3, 5, 4, 2, one, one, one, one, None]
    for position, value in ((0, None), (1, None), (2, None), (3, -1), (4, 0), (4, 6), (5, -1), (5, 5), (6, 0), (7, -1),
                            (7, big), (8, 0), (9, None), (10, None), (11, None), (12, None)):
        args = list(good)
        args[position] = value
        assert sums(*args) == bad, (position, value)
    assert b"rank_sums" in lib.icv_last_error()
    args = list(good)
    args[5] = 0
    assert sums(*args) == _lib.ICV_OK  # nothing stored in the tile: nothing runs
    finish = lib.icv_rank_finish
    good = [one, one, one, one, 2, 5, 4, one, one, None]
    for position, value in ((0, None), (1, None), (2, None), (3, None), (4, -1), (5, 0), (6, -1), (6, big), (7, None),
                            (8, None)):
        args = list(good)
        args[position] = value
        assert finish(*args) == bad, (position, value)
    assert b"rank_finish" in lib.icv_last_error()
    assert finish(None, None, None, None, 0, 5, 4, None, None, None) == _lib.ICV_OK  # no groups: nothing runs

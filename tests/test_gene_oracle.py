"""CPU tests of ``tests/_gene_oracle.py`` and ``tests/_gene_cases.py`` (they need the built host library for the plans'
run tables, like ``test_host_plan.py``):

* ``gene_layer`` -- the contract from the run tables -- equals the layer assembled from the end-to-end oracle's
  ``gene_values_from_windows`` per chromosome, ``np.median`` and the threshold;
* every planted case of ``tests/test_gpu_gene_values_edges.py`` reaches the branch it is named for
  (``median_path`` / ``row_median_path``, the run tables), proven here before any GPU run.
"""
import numpy as np
import pytest

import _gene_cases as gc
import _gene_oracle as go
import cases
from infercnvpy_amd._plan import GenePlan
from oracle import infercnv_oracle as O


@pytest.fixture(scope="module")
def runs_of():
    cache = {}

    def get(name):
        if name not in cache:
            plan = gc.make_plan(name)
            cache[name] = (plan.gene_runs(), plan.n_windows, plan.n_cols_all)
            plan.close()
        return cache[name]
    return get


@pytest.mark.parametrize("genes,window,step", [
    ([57, 23, 9], 10, 3), ([120, 40], 25, 5), ([64, 64, 5], 8, 4), ([33], 11, 1), ([200, 90, 12], 100, 10),
    ([75, 31], 6, 7),
])
@pytest.mark.parametrize("with_thr", [False, True])
def test_gene_layer_is_the_oracles_layer(genes, window, step, with_thr):
    v = cases.synthetic_var(genes, extra=(("chrX", 7), (None, 3)))
    chrom, start = v["chromosome"], v["start"]
    plan = GenePlan(chrom, start, window_size=window, step=step)
    runs, n_w, n_cols = plan.gene_runs(), plan.n_windows, len(chrom)
    keep = ~plan.var_mask
    ch, st = chrom[keep], start[keep]
    kept_idx = np.flatnonzero(keep)
    rows = 7
    win = np.random.RandomState(5).standard_normal((rows, n_w))
    win[3, n_w // 2] = np.nan
    thr = np.array([0.3, 0.05, 0.6]) if with_thr else None
    chunksize, row_phase = 3, 1
    cols, vals = [], []
    for c in O.used_chromosomes(ch):
        order = O.chromosome_gene_order(ch, st, c)
        w0 = int(plan.chr_pos[c])
        n_wc = O.smooth_segment(np.zeros((1, len(order))), window, step).shape[1]
        gv = O.gene_values_from_windows(win[:, w0:w0 + n_wc], len(order), window, step)
        covered = ~np.isnan(O.gene_values_from_windows(np.zeros((1, n_wc)), len(order), window, step)[0])
        cols.append(kept_idx[order[covered]])
        vals.append(gv[:, covered])
    plan.close()
    cols, vals = np.concatenate(cols), np.hstack(vals)
    vals = vals - np.median(vals, axis=1)[:, None]
    if with_thr:
        for i in range(rows):
            vals[i, np.abs(vals[i]) < thr[(i + row_phase) // chunksize]] = 0.0
    want = np.full((rows, n_cols), np.nan)
    want[:, cols] = vals
    got = go.gene_layer(runs, win, n_cols, thr=thr, chunksize=chunksize, row_phase=row_phase)
    assert np.isnan(got[3, cols]).all() and not np.isnan(got[2, cols]).any() and np.isnan(got).any(axis=0).sum() > 0
    go.same_bytes(got, want)


def test_same_bytes_ignores_only_the_sign_of_zero():
    a = np.array([[0.0, -0.0, np.nan, 1.0]])
    go.same_bytes(a, np.array([[-0.0, 0.0, np.nan, 1.0]]))
    with pytest.raises(AssertionError):
        go.same_bytes(a, np.array([[0.0, 0.0, np.nan, np.nextafter(1.0, 2.0)]]))
    with pytest.raises(AssertionError):
        go.same_bytes(a, np.array([[0.0, 0.0, 0.0, 1.0]]))
    with pytest.raises(AssertionError):
        go.same_bytes(a, np.array([[0.0, 5e-324, np.nan, 1.0]]))


@pytest.mark.parametrize("name", ["odd", "even"])
def test_planted_medians_cover_what_they_are_named_for(name, runs_of):
    runs, n_w, _ = runs_of(name)
    n = len(runs["first"])
    assert n == n_w and (runs["count"] == 1).all() and (runs["genes"] == 1).all()
    assert sorted(runs["first"]) == list(range(n)) and n % 2 == (name == "odd")
    pats = {**gc.planted(n), **gc.subnormal(n)}
    names, mat = gc.shuffled(pats)
    seen = {}
    for k, row in zip(names, mat):
        assert len(row) == n
        path = go.median_path(row[runs["first"]], runs["genes"])
        pats[k][1](path)
        seen[k] = path
        srt = np.sort(np.repeat(row[runs["first"]], runs["genes"]))
        assert path["v1"] == srt[(n - 1) // 2] and path["v2"] == srt[n // 2], k  # the restatement itself is right
    # the list of the issue, by ending
    assert seen["crowded200"]["counts"][0] > 64                                    # a level-0 bin with more than 64 values
    assert len(seen["nested"]["counts"]) >= 3                                      # >= 3 levels
    assert seen["all_equal"]["end"] == "equal" and not seen["all_equal"]["counts"]  # "equal" at level 0
    assert seen["tie"]["end"] == "equal" and len(seen["tie"]["counts"]) >= 1       # ... and at a level >= 1
    assert seen["cand64"]["counts"] == [64] and seen["cand65"]["counts"][0] == 65
    if name == "even":
        assert seen["mid_two_bins"]["end"] == "candidates+next_above"
        assert seen["tie_k2_past"]["end"] == "equal+next_above" and seen["mid_one_bin"]["end"] == "candidates"
        assert len(seen["tie_k2_past_same_bin"]["counts"]) == 2


def test_weighted_plan_has_runs_of_different_lengths_and_medians_that_need_them(runs_of):
    runs, n_w, _ = runs_of("weighted")
    assert (runs["count"] == 1).all() and len(set(runs["genes"])) > 1 and set(runs["genes"]) >= set(range(1, 9))
    win = gc.dyadic(12, n_w, seed=3)
    differ = 0
    for row in win:
        val = go.run_values(runs, row)
        wm = np.median(np.repeat(val, runs["genes"]))
        path = go.median_path(val, runs["genes"])
        assert (path["v1"] + path["v2"]) / 2.0 == wm
        differ += wm != np.median(val)
    assert differ >= 6


def test_heavy_plans_have_a_run_of_more_than_255_genes(runs_of):
    for name, w in (("heavy", 6), ("heavy3", 3)):
        runs, n_w, _ = runs_of(name)
        assert n_w == w and runs["genes"].max() == 300 > 255 and (runs["count"] == 1).all()
    runs, n_w, _ = runs_of("light4")
    assert n_w == 4 and runs["genes"].max() <= 255
    # their rows: every assignment of three values to the runs.  The median element is found among the candidates of
    # bin 0, of bin 2047 (v == hi: the clamp) and of bins between; all-equal rows end at level 0
    for name in ("heavy", "heavy3", "light4"):
        runs, n_w, _ = runs_of(name)
        seen = set()
        for row in gc.small_rows(n_w):
            p = go.median_path(go.run_values(runs, row), runs["genes"])
            seen.add((p["end"].split("+")[0], p["bins"][-1] if p["bins"] else None))
        assert {("candidates", 0), ("candidates", 2047), ("equal", None)} <= seen, seen
        assert any(b not in (0, 2047, None) for _, b in seen)


@pytest.mark.parametrize("name", ["rm_even", "rm_odd"])
def test_row_median_cases_cover_what_they_are_named_for(name, runs_of):
    runs, n_w, _ = runs_of(name)
    n = len(runs["first"])
    assert n == n_w > 1024 + 400 and (runs["count"] == 1).all() and (runs["genes"] == 1).all()
    pats = gc.row_median_planted(n)
    names, mat = gc.shuffled(pats)
    ends = set()
    for k, row in zip(names, mat):
        path = go.row_median_path(row[runs["first"]])
        pats[k][1](path)
        ends.add(path["end"])
        go.median_path(row[runs["first"]], runs["genes"])  # (the fused kernel's search ends as well)
    assert ends == ({"adjacent", "candidates", "separated"} if name == "rm_even" else {"adjacent", "candidates"})


def test_run_sum_plans_cover_every_count_and_their_sums_depend_on_the_order(runs_of):
    runs, n_w, _ = runs_of("sum128")
    assert set(runs["count"]) >= set(range(1, 129)) and runs["count"].max() == 128
    runs3, n_w3, _ = runs_of("sum300")
    assert runs3["count"].max() == 300 > 128 and runs3["genes"].sum() > 1024
    # the recursion above 128 splits at multiples of 8: counts that are none are there
    assert any(c > 128 and (c // 2) % 8 for c in runs3["count"])
    for r, w, seed in ((runs, n_w, 21), (runs3, n_w3, 22)):
        win = gc.order_sensitive(3, w, seed)
        differ = total = 0
        for row in win:
            differ += int((go.run_values(r, row) != gc.sequential_run_values(r, row)).sum())
            total += len(r["first"])
        assert 3 * differ >= total, (differ, total)


def test_filter_rows_sit_on_the_threshold(runs_of):
    runs, n_w, n_cols = runs_of("odd")
    rows, chunksize = 20, 8
    win = gc.filter_rows(rows, n_w)
    assert (np.median(win, axis=1) == gc.FILTER_MED).all()
    base = go.gene_layer(runs, win, n_cols, thr=gc.FILTER_THR, chunksize=chunksize, row_phase=0)
    moved = go.gene_layer(runs, win, n_cols, thr=gc.FILTER_THR, chunksize=chunksize, row_phase=3)
    none = go.gene_layer(runs, win, n_cols)
    for i in range(rows):
        t = gc.FILTER_THR[i // chunksize]
        a = none[i][~np.isnan(none[i])]
        kept = base[i][~np.isnan(base[i])]
        # |a| == thr (the planted values, and neighbours whose difference rounds onto it): kept by the strict <
        assert (np.abs(a) == t).sum() >= 2 and (np.abs(kept) == t).sum() == (np.abs(a) == t).sum()
        below = np.abs(a) < t
        assert below.sum() > 2 and np.abs(a[below]).max() >= t - 2.0 ** -52 and (kept[below] == 0).all()
        assert (np.abs(a) > t).any() and np.abs(a[np.abs(a) > t]).min() <= t + 2.0 ** -52
        # a row in another chunk under row_phase 3 comes out differently
        if (i + 3) // chunksize != i // chunksize:
            assert not np.array_equal(np.nan_to_num(base[i]), np.nan_to_num(moved[i]))

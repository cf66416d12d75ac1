"""tl/_groups.py on the CPU: the group table that tl.cnv_segments and tl.cnv_pseudobulk share gives what each of them formed
with its own lines before (kept below, word for word, as the two references), on the label columns where they could part."""
import numpy as np
import pandas as pd
import pytest

COLUMNS = {
    "plain labels with None and NaN": ["b", None, "a", "b", np.nan, "c", "a", "b"],
    "categorical with an unused category": pd.Categorical(list("xzzxz"), categories=list("xyz")),
    "categorical with every code -1": pd.Categorical([None] * 4, categories=list("pq")),
    "one cell per group": [3, 1, 2, 0],
    "numbers with a NaN": [2.5, np.nan, 2.5, 1.0],
}


def _adata(labels):
    from infercnvpy_amd._compat import SimpleAnnData

    return SimpleAnnData(np.zeros((len(labels), 2), dtype=np.float32), obs=pd.DataFrame({"clone": labels}))


def _segments_before(codes, n_groups):
    n = codes.shape[0]
    listed = codes >= 0
    rows = np.argsort(codes, kind="stable")[int(n - listed.sum()):].astype(np.int64)
    n_cells = np.bincount(codes[listed], minlength=n_groups).astype(np.int64)
    group_ptr = np.zeros(n_groups + 1, dtype=np.int64)
    group_ptr[1:] = np.cumsum(n_cells)
    return rows, group_ptr, n_cells


def _pseudobulk_before(codes, n_groups, kept):
    sizes = np.bincount(codes[codes >= 0], minlength=n_groups).astype(np.int64)
    new_code = np.full(n_groups + 1, -1, dtype=np.int64)
    new_code[kept] = np.arange(kept.shape[0])
    codes = new_code[codes]
    rows = np.argsort(codes, kind="stable")[int((codes < 0).sum()):].astype(np.int64)
    group_ptr = np.zeros(kept.shape[0] + 1, dtype=np.int64)
    group_ptr[1:] = np.cumsum(sizes[kept])
    return rows, group_ptr, sizes[kept]


def _check(got, want, codes):
    """Same arrays and dtypes as the reference, and the table's own properties."""
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.dtype == w.dtype and np.array_equal(g, w)
    rows, group_ptr, sizes = got
    assert group_ptr[0] == 0 and group_ptr[-1] == len(rows) and np.array_equal(np.diff(group_ptr), sizes)
    for g in range(len(sizes)):
        mine = rows[group_ptr[g]:group_ptr[g + 1]]
        assert np.all(np.diff(mine) > 0) and np.all(codes[mine] == g)


@pytest.mark.parametrize("name", list(COLUMNS))
def test_all_groups_as_tl_cnv_segments_listed_them(name):
    from infercnvpy_amd.tl._groups import group_codes, group_table

    codes, groups = group_codes(_adata(COLUMNS[name]), "clone")
    assert codes.dtype == np.int64 and codes.shape == (len(COLUMNS[name]),)
    got = group_table(codes, len(groups))
    _check(got, _segments_before(codes, len(groups)), codes)
    assert np.array_equal(got[2], np.bincount(codes[codes >= 0], minlength=len(groups)))  # (groups of no cells stay)


def test_the_codes_keep_unused_categories_and_mark_missing_labels():
    from infercnvpy_amd.tl._groups import group_codes

    codes, groups = group_codes(_adata(COLUMNS["plain labels with None and NaN"]), "clone")
    assert codes.tolist() == [0, -1, 1, 0, -1, 2, 1, 0] and groups.tolist() == ["b", "a", "c"]
    codes, groups = group_codes(_adata(COLUMNS["categorical with an unused category"]), "clone")
    assert codes.tolist() == [0, 2, 2, 0, 2] and groups.tolist() == ["x", "y", "z"]
    codes, groups = group_codes(_adata(COLUMNS["categorical with every code -1"]), "clone")
    assert codes.tolist() == [-1] * 4 and groups.tolist() == ["p", "q"]


@pytest.mark.parametrize("name", list(COLUMNS))
@pytest.mark.parametrize("min_cells", [1, 2, 3])
def test_kept_groups_as_tl_cnv_pseudobulk_listed_them(name, min_cells):
    from infercnvpy_amd.tl._groups import group_codes, group_table
    from infercnvpy_amd.tl._pseudobulk import group_lists

    ad = _adata(COLUMNS[name])
    codes, groups = group_codes(ad, "clone")
    sizes = np.bincount(codes[codes >= 0], minlength=len(groups))
    kept = np.flatnonzero(sizes >= min_cells)
    if kept.shape[0] == 0:  # an empty keep: the table is empty, and tl.cnv_pseudobulk raises before it forms one
        rows, group_ptr, n_cells = group_table(codes, len(groups), keep=kept)
        assert rows.shape == (0,) and group_ptr.tolist() == [0] and n_cells.shape == (0,)
        with pytest.raises(ValueError, match=f"no group of `clone` has min_cells={min_cells} cells"):
            group_lists(ad, "clone", len(codes), min_cells)
        return
    want = _pseudobulk_before(codes, len(groups), kept)
    renumbered = np.append(np.full(len(groups), -1), -1)
    renumbered[kept] = np.arange(len(kept))
    _check(group_table(codes, len(groups), keep=kept), want, renumbered[codes])
    labels, n_cells, dropped, rows, group_ptr = group_lists(ad, "clone", len(codes), min_cells)
    assert labels.tolist() == groups[kept].tolist() and dropped == [groups[g] for g in np.flatnonzero(sizes < min_cells)]
    _check((rows, group_ptr, n_cells), want, renumbered[codes])


def test_keep_that_drops_the_first_and_the_last_group():
    from infercnvpy_amd.tl._groups import group_table

    codes = np.asarray([3, 0, 1, -1, 2, 1, 0, 3, 2, 1], dtype=np.int64)
    keep = np.asarray([1, 2])
    got = group_table(codes, 4, keep=keep)
    _check(got, _pseudobulk_before(codes, 4, keep), np.asarray([-1, -1, 0, -1, 1, 0, -1, -1, 1, 0]))
    assert got[0].tolist() == [2, 5, 9, 4, 8] and got[1].tolist() == [0, 3, 5] and got[2].tolist() == [3, 2]

"""The arguments of tl.cnv_silhouette and of the two entry points behind it that are refused before any GPU work: the
exception's type and the rule it names.  No test here needs a device."""
import ctypes

import numpy as np
import pandas as pd
import pytest

INVALID, UNSUPPORTED = 1, 2  # ICV_ERR_INVALID, ICV_ERR_UNSUPPORTED
ONE = ctypes.c_void_p(16)    # never dereferenced: every call below fails in the argument checks


def _adata(x=None, labels=None):
    from infercnvpy_amd._compat import SimpleAnnData

    x = np.random.default_rng(0).normal(0, 1, (6, 3)).astype(np.float32) if x is None else x
    labels = ["a", "a", "b", "b", "c", "c"][:x.shape[0]] if labels is None else labels
    ad = SimpleAnnData(np.zeros((x.shape[0], 2), dtype=np.float32), obs=pd.DataFrame({"cnv_leiden": labels}))
    ad.obsm["X_cnv_pca"] = x
    return ad


def _no_rep():
    ad = _adata()
    del ad.obsm["X_cnv_pca"]
    return ad


def _with(value):
    x = np.ones((6, 3))
    x[4, 1] = value
    return _adata(x)


CASES = [
    ("no_representation", _no_rep, {}, KeyError, "tl.cnv_silhouette: X_cnv_pca not found in adata.obsm. Did you run `tl.pca`?"),
    ("other_rep", _adata, {"use_rep": "umap"}, KeyError, "X_umap not found in adata.obsm"),
    ("no_column", _adata, {"groupby": "clone"}, KeyError, "`clone` not found in `adata.obs`"),
    ("no_leiden", lambda: _adata(labels=None), {"groupby": "cnv_leiden2"}, KeyError, "`cnv_leiden2` not found"),
    ("not_2d", lambda: _adata_raw(np.zeros(6)), {}, ValueError, "X_cnv_pca must be 2-D"),
    ("no_components", lambda: _adata(np.zeros((6, 0))), {}, ValueError, "empty matrix of shape (6, 0)"),
    ("too_many_components", lambda: _adata(np.zeros((6, 257))), {}, ValueError,
     "X_cnv_pca has 257 components; at most 256 are supported"),
    ("one_group", lambda: _adata(labels=["a"] * 6), {}, ValueError, "at least two groups with cells, got 1"),
    ("one_group_and_missing", lambda: _adata(labels=["a", "a", None, "a", None, "a"]), {}, ValueError,
     "at least two groups with cells, got 1"),
    ("one_used_category", lambda: _adata(labels=pd.Categorical(["a"] * 6, categories=["a", "b"])), {}, ValueError,
     "at least two groups with cells, got 1"),
    ("nan", lambda: _with(np.nan), {}, ValueError, "X_cnv_pca has non-finite values"),
    ("inf", lambda: _with(-np.inf), {}, ValueError, "X_cnv_pca has non-finite values"),
    ("shift_below_0", lambda: _with(2.0 ** 60), {}, ValueError, "too large for an exact int64 sum of distances"),
]


def _adata_raw(x):
    ad = _adata()
    ad.obsm["X_cnv_pca"] = x
    return ad


@pytest.mark.parametrize("name,make,kwargs,exc,text", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_come_before_any_gpu_work(name, make, kwargs, exc, text):
    import infercnvpy_amd as cnv

    ad = make()
    with pytest.raises(exc) as info:
        cnv.tl.cnv_silhouette(ad, **kwargs)
    assert text in str(info.value)
    assert "cnv_silhouette" not in ad.obs.columns and "cnv_silhouette" not in ad.uns


def test_the_no_leiden_hint():
    import infercnvpy_amd as cnv

    ad = _adata()
    ad.obs = ad.obs.rename(columns={"cnv_leiden": "other"})
    with pytest.raises(KeyError, match="Did you run `tl.leiden`"):
        cnv.tl.cnv_silhouette(ad)


def test_shift_rule_is_the_oracles():
    import _silhouette_oracle as so
    from infercnvpy_amd.tl._silhouette import distance_shift

    for m in (0.0, 1e-300, 0.5, 1.0, 3.7, 2047.9, 2.0 ** 20, 2.0 ** 45, 2.0 ** 60):
        for largest in (1, 2, 66, 4095, 10 ** 6):
            for c in (1, 2, 3, 50, 255, 256):
                assert distance_shift(m, largest, c) == so.shift_of(m, largest, c)


def test_tile_table_never_straddles_a_group_and_chunks_cover_it():
    from infercnvpy_amd import _engine

    tj = _engine.SILHOUETTE_TILE_J
    group_ptr = np.cumsum([0, 1, 0, tj - 1, tj, tj + 1, 0, 3 * tj + 5])
    for n_chunks in (1, 2, 3, 7, 100):
        tiles, chunk_ptr = _engine.silhouette_tiles(group_ptr, n_chunks)
        start, count, group = tiles
        assert (count >= 1).all() and (count <= tj).all()
        assert (start >= group_ptr[group]).all() and (start + count <= group_ptr[group + 1]).all()
        assert np.concatenate([np.arange(s, s + c) for s, c in zip(start, count)]).tolist() == list(range(group_ptr[-1]))
        assert chunk_ptr[0] == 0 and chunk_ptr[-1] == tiles.shape[1] and (np.diff(chunk_ptr) >= 1).all()
        assert chunk_ptr.shape[0] - 1 == min(n_chunks, tiles.shape[1])


def _entry_cases():
    good = dict(x=ONE, dtype=0, n_rows=10, n_comp=4, ld=4, rows=ONE, n_listed=10, i0=0, i1=10, tiles=ONE, n_tiles=1,
                chunk_ptr=ONE, n_chunks=1, n_groups=2, shift=40, dist_exp=5, sums=ONE, flags=ONE)
    bad = [("dtype", {"dtype": 2}), ("no_components", {"n_comp": 0}), ("components", {"n_comp": 257}),
           ("ld", {"ld": 3}), ("i0_not_a_tile", {"i0": 1}), ("i1_beyond", {"i1": 11}), ("i1_below_i0", {"i0": 64, "i1": 10}),
           ("no_groups", {"n_groups": 0}), ("shift_41", {"shift": 41}), ("shift_negative", {"shift": -1}),
           ("null_x", {"x": None}), ("null_rows", {"rows": None}), ("null_sums", {"sums": None}),
           ("null_flags", {"flags": None}), ("null_tiles", {"tiles": None}), ("null_chunks", {"chunk_ptr": None})]
    return good, bad


@pytest.mark.parametrize("name,change", _entry_cases()[1], ids=[c[0] for c in _entry_cases()[1]])
def test_sums_entry_refuses_bad_arguments(name, change):
    from infercnvpy_amd import _lib

    args = dict(_entry_cases()[0], **change)
    assert _lib.load().icv_silhouette_sums(*args.values(), None) == INVALID
    assert b"silhouette_sums" in _lib.load().icv_last_error()


def test_sums_entry_takes_an_empty_range_of_positions():
    from infercnvpy_amd import _lib

    args = dict(_entry_cases()[0], i1=0, x=None, rows=None, sums=None)  # (nothing is read, cleared or launched)
    assert _lib.load().icv_silhouette_sums(*args.values(), None) == 0


@pytest.mark.parametrize("name,change", [("i1_below_i0", {"i0": 5, "i1": 4}), ("no_groups", {"n_groups": 0}),
                                         ("shift_41", {"shift": 41}), ("null_sums", {"sums": None}),
                                         ("null_out", {"nearest": None})])
def test_finish_entry_refuses_bad_arguments(name, change):
    from infercnvpy_amd import _lib

    args = dict(dict(sums=ONE, i0=0, i1=10, group_ptr=ONE, n_groups=2, shift=40, s=ONE, a=ONE, b=ONE, nearest=ONE), **change)
    assert _lib.load().icv_silhouette_finish(*args.values(), None) == INVALID
    assert b"silhouette_finish" in _lib.load().icv_last_error()
